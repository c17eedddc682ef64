// hb_ldqplan.hpp — what one batch of hb_ldm_window_var (hb_ldquad.hip) is launched with, decided in one place. Plain C++ and
// host-testable (tests/test_ldpve_host.py compiles it alone). From the effects of up to 8 records and the window map it makes
//     the list      the marker columns that carry a non-zero effect in any record of the batch, sorted by window id and, within a window, by
//                   marker index: the columns the pass visits, one wave each, and the order in which a window's columns are added
//     the segments  (window, first entry, count) for every window that has an entry, in window order: a window without one is never visited
//     the table     aw[i][r], the m x 8 effects row by row (records past nr: 0.0), so that one stored entry (i, j) finds the 8 effects of its
//                   row in 64 contiguous bytes, and win[i]: marker i's window id where the row has a non-zero effect in the batch, 0 where it
//                   has none — such a row contributes (alpha != 0 ? V alpha : 0.0) = 0.0 to every sum and is passed over without its effects
//                   being read
// The grid is one wave per list entry: it needs no decision.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

constexpr int HB_LDQ_RB = 8; // records per batch (hb_ctx_window_var's)

struct hb_ldqseg {
    int32_t window = 0; // 0-based
    int32_t first = 0, count = 0;
};

struct hb_ldqplan {
    std::string error;          // non-empty: refused, nothing else is valid
    int nr = 0;
    std::vector<int32_t> idx;   // nnz
    std::vector<hb_ldqseg> segs;
    std::vector<double> aw;     // m x HB_LDQ_RB
    std::vector<uint32_t> win;  // m
};

// what is refused of a call's arguments, for all its R records at once (empty: nothing), so that no batch runs before a later one is refused
inline std::string hb_ldq_check(const double *A, int64_t ldA, int m, int R, const uint32_t *windindx, int nw)
{
    if (!A || !windindx) return "null argument";
    if (m < 1 || nw < 1 || ldA < m) return "m and nw must be >= 1 and ldA >= m";
    if (R < 1) return "no record (R must be >= 1)";
    for (int j = 0; j < m; j++)
        if (windindx[j] < 1u || windindx[j] > (uint32_t)nw)
            return "windindx must hold window ids in 1 .. nw (marker " + std::to_string(j + 1) + " has " + std::to_string(windindx[j]) + ")";
    for (int r = 0; r < R; r++)
        for (int j = 0; j < m; j++)
            if (!std::isfinite(A[(size_t)r * ldA + j]))
                return "the effects must be finite (marker " + std::to_string(j + 1) + ", record " + std::to_string(r + 1) + ")";
    return std::string();
}

// A: m x nr column-major effects (leading dimension ldA >= m), windindx: m ids in 1 .. nw. The call's arguments are hb_ldq_check's to refuse,
// once for all records; a batch refuses its size alone and, in the pass it makes anyway, a window id it could not index with.
inline hb_ldqplan hb_ldqplan_of(const double *A, int64_t ldA, int m, int nr, const uint32_t *windindx, int nw)
{
    hb_ldqplan p;
    if (nr < 1 || nr > HB_LDQ_RB) { p.error = "a batch holds 1 .. 8 records"; return p; }
    if (!A || !windindx || m < 1 || nw < 1 || ldA < m) { p.error = "bad argument"; return p; }
    p.nr = nr;
    p.aw.assign((size_t)m * HB_LDQ_RB, 0.0);
    p.win.assign((size_t)m, 0u);
    // the entries of every window, counted, then placed in marker order (a counting sort: stable)
    std::vector<int32_t> start((size_t)nw + 1, 0);
    for (int j = 0; j < m; j++) {
        const uint32_t w = windindx[j];
        if (w < 1u || w > (uint32_t)nw) { p.error = "windindx must hold window ids in 1 .. nw"; return p; }
        bool nz = false;
        for (int r = 0; r < nr; r++) {
            const double a = A[(size_t)r * ldA + j];
            p.aw[(size_t)j * HB_LDQ_RB + r] = a;
            nz |= a != 0.0;
        }
        if (nz) { p.win[j] = w; start[w]++; }
    }
    for (int w = 0; w < nw; w++) start[w + 1] += start[w];
    p.idx.resize((size_t)start[nw]);
    std::vector<int32_t> fill(start.begin(), start.end() - 1);
    for (int j = 0; j < m; j++)
        if (p.win[j]) p.idx[fill[p.win[j] - 1]++] = j;
    for (int w = 0; w < nw; w++) {
        if (start[w + 1] == start[w]) continue;
        hb_ldqseg s;
        s.window = w, s.first = start[w], s.count = start[w + 1] - start[w];
        p.segs.push_back(s);
    }
    return p;
}
