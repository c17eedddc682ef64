// hb_cholplan.hpp — what hb_chol.hip's three stages (dpotrf, dtrtri, dlauum on an n x n fp64 device matrix) are launched with,
// decided in one place. Plain C++ and host-testable (tests/test_chol_host.py compiles it alone; hb_chol_plan hands it out): the panel width, the
// work buffer's leading dimension, every panel step of the factorisation with its tile counts, and the bytes a call allocates.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

constexpr int HB_CHOL_SB = 256; // super-block of the factor's inverse: its diagonal super-blocks are inverted first, then block columns of this width
constexpr int HB_CHOL_NB = 64;  // panel width = tile edge of the matrix-core kernels (hb_mma.hpp: a workgroup's 64 x 64 tile, four waves of 32 x 32)

// one panel of the right-looking factorisation: columns [k0, k0 + width)
struct hb_cholstep {
    int k0 = 0, width = 0;
    int row_tiles = 0;       // 64-row tiles of the panel below its diagonal block: the workgroups of the panel solve
    long long tri_tiles = 0; // 64 x 64 tiles of the lower triangle of the trailing matrix: the workgroups of the update
};

struct hb_cholplan {
    int n = 0, nb = HB_CHOL_NB;
    int blocks = 0;             // block columns: ceil(n / nb)
    int super_blocks = 0;       // ceil(n / HB_CHOL_SB)
    int64_t ldw = 0;            // leading dimension of the work buffer and of the panel buffer: n rounded up to even, so columns start on 16 bytes
    size_t work_bytes = 0;      // ldw x n doubles: the copy of the lower triangle that hb_spd_inverse factors and inverts
    size_t panel_bytes = 0;     // ldw x HB_CHOL_SB doubles: a super-block column of the inverse before its last multiplication (hb_chol_invert_factor)
    size_t info_bytes = 0;      // the device word the factorisation records its failing minor in (16 bytes, one allocation)
    size_t factor_bytes = 0;    // hb_chol_factor allocates:        info
    size_t invert_bytes = 0;    // hb_chol_invert_factor allocates: info + panel
    size_t inverse_bytes = 0;   // hb_spd_inverse allocates:        info + panel + work
    std::vector<hb_cholstep> steps;
};

inline hb_cholplan hb_cholplan_of(int n)
{
    hb_cholplan p;
    if (n < 1) return p;
    constexpr int NB = HB_CHOL_NB;
    p.n = n;
    p.blocks = (n + NB - 1) / NB;
    p.super_blocks = (n + HB_CHOL_SB - 1) / HB_CHOL_SB;
    p.ldw = (int64_t)n + (n & 1);
    p.work_bytes = sizeof(double) * (size_t)p.ldw * (size_t)n;
    p.panel_bytes = sizeof(double) * (size_t)p.ldw * (size_t)HB_CHOL_SB;
    p.info_bytes = 16;
    p.factor_bytes = p.info_bytes;
    p.invert_bytes = p.info_bytes + p.panel_bytes;
    p.inverse_bytes = p.invert_bytes + p.work_bytes;
    p.steps.reserve((size_t)p.blocks);
    for (int k0 = 0; k0 < n; k0 += NB) {
        hb_cholstep s;
        s.k0 = k0;
        s.width = n - k0 < NB ? n - k0 : NB;
        const int below = n - k0 - s.width; // rows under the diagonal block (only a full-width panel has any)
        s.row_tiles = (below + NB - 1) / NB;
        s.tri_tiles = (long long)s.row_tiles * (s.row_tiles + 1) / 2;
        p.steps.push_back(s);
    }
    return p;
}
