// hb_pveplan.hpp — what one batch of hb_ctx_window_var (hb_pve.hip) is launched with, decided in one place. Plain C++ and
// host-testable (tests/test_pve_host.py compiles it alone; hb_pve_plan hands it out). From the effects of up to 8 records, the window map and
// the column sums it makes
//     the list      the marker columns that carry a non-zero effect in any record of the batch, sorted by window id and, within a window, by
//                   marker index — the order of a (row, record) pair's fma chain, which therefore does not depend on what else is in the batch —,
//                   with the 8 effects of each entry (records past nr: 0.0)
//     the segments  (window, first entry, count) for every window that has an entry, in window order: a window without one is never visited
//     the shifts    c[w][r] = sum_e (s1[j_e] / n) alpha[e][r] in list order, the window's mean breeding value: k_window_var sums g - c and its
//                   square, and for ANY c sum (g - c)^2 - (sum (g - c))^2 / n is the centred sum of squares; c only keeps the two terms small
//     the grid      row blocks of HB_PVE_ROWS rows x chunks of whole segments, the chunks balanced by entry count. Row blocks alone (49 at
//                   n = 50 000) would leave most compute units idle; the chunks bring the grid to HB_PVE_FILL workgroups per unit or to one
//                   segment per chunk, whichever comes first. The row blocks depend on n alone: the partial sums of a (window, record) pair are
//                   the same whatever the chunks are.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

constexpr int HB_PVE_RB = 8;       // records per batch (hb_ctx_matmul's)
constexpr int HB_PVE_ROWS = 1024;  // rows of a workgroup: 256 threads x 4 rows
constexpr int HB_PVE_FILL = 4;     // workgroups per compute unit the chunks aim for

struct hb_pveseg {
    int32_t window = 0; // 0-based
    int32_t first = 0, count = 0;
};

struct hb_pvechunk {
    int32_t first = 0, count = 0; // segments
};

struct hb_pveplan {
    std::string error;             // non-empty: refused, nothing else is valid
    int nr = 0;
    int row_blocks = 0;
    std::vector<int32_t> idx;      // nnz
    std::vector<double> val;       // nnz x HB_PVE_RB
    std::vector<hb_pveseg> segs;
    std::vector<double> shift;     // segs x HB_PVE_RB
    double total_shift[HB_PVE_RB]; // the shift of the one all-entries segment behind var(X alpha): the same sum over the whole list
    std::vector<hb_pvechunk> chunks;
};

// A: m x nr column-major effects (leading dimension ldA >= m), windindx: m ids in 1 .. nw, s1: m column sums over the n individuals,
// ld: rows of a resident column (>= n, a multiple of 4)
inline hb_pveplan hb_pveplan_of(const double *A, int64_t ldA, int m, int nr, const uint32_t *windindx, int nw, const double *s1, int n, int64_t ld,
                                int num_cus)
{
    hb_pveplan p;
    for (int r = 0; r < HB_PVE_RB; r++) p.total_shift[r] = 0.0;
    if (!A || !windindx || !s1) { p.error = "null argument"; return p; }
    if (m < 1 || nw < 1 || ldA < m) { p.error = "m and nw must be >= 1 and ldA >= m"; return p; }
    if (nr < 1 || nr > HB_PVE_RB) { p.error = "a batch holds 1 .. 8 records"; return p; }
    if (n < 2) { p.error = "a variance needs n >= 2 individuals"; return p; }
    if (ld < n || ld % 4) { p.error = "ld must be >= n and a multiple of 4"; return p; }
    if (num_cus < 1) num_cus = 1;
    p.nr = nr;
    p.row_blocks = (n + HB_PVE_ROWS - 1) / HB_PVE_ROWS;
    // the entries of every window, counted, then placed in marker order (a counting sort: stable)
    std::vector<int32_t> start((size_t)nw + 1, 0);
    std::vector<uint8_t> any((size_t)m, 0);
    for (int j = 0; j < m; j++) {
        const uint32_t w = windindx[j];
        if (w < 1u || w > (uint32_t)nw) { p.error = "windindx must hold window ids in 1 .. nw (marker " + std::to_string(j + 1) + " has " + std::to_string(w) + ")"; return p; }
        bool nz = false;
        for (int r = 0; r < nr; r++) {
            const double a = A[(size_t)r * ldA + j];
            if (!std::isfinite(a)) { p.error = "the effects must be finite (marker " + std::to_string(j + 1) + ", record " + std::to_string(r + 1) + ")"; return p; }
            nz |= a != 0.0;
        }
        if (nz) { any[j] = 1; start[w]++; }
    }
    for (int w = 0; w < nw; w++) start[w + 1] += start[w];
    const int nnz = start[nw];
    p.idx.resize((size_t)nnz);
    p.val.assign((size_t)nnz * HB_PVE_RB, 0.0);
    std::vector<int32_t> fill(start.begin(), start.end() - 1);
    for (int j = 0; j < m; j++) {
        if (!any[j]) continue;
        const int e = fill[windindx[j] - 1]++;
        p.idx[e] = j;
        for (int r = 0; r < nr; r++) p.val[(size_t)e * HB_PVE_RB + r] = A[(size_t)r * ldA + j];
    }
    for (int w = 0; w < nw; w++) {
        if (start[w + 1] == start[w]) continue;
        hb_pveseg s;
        s.window = w, s.first = start[w], s.count = start[w + 1] - start[w];
        p.segs.push_back(s);
    }
    const int nseg = (int)p.segs.size();
    p.shift.assign((size_t)nseg * HB_PVE_RB, 0.0);
    for (int si = 0; si < nseg; si++) {
        const hb_pveseg &s = p.segs[si];
        for (int e = s.first; e < s.first + s.count; e++) {
            const double mean = s1[p.idx[e]] / (double)n;
            for (int r = 0; r < nr; r++) {
                p.shift[(size_t)si * HB_PVE_RB + r] += mean * p.val[(size_t)e * HB_PVE_RB + r];
                p.total_shift[r] += mean * p.val[(size_t)e * HB_PVE_RB + r];
            }
        }
    }
    if (!nseg) return p;
    // chunks of whole segments: a chunk takes segments until it holds its share of the entries that are left — what is left divided by the
    // chunks that are left, so that one heavy window does not starve the chunks after it —, at least one and never so many that a later
    // chunk would be left empty
    const int want = (HB_PVE_FILL * num_cus + p.row_blocks - 1) / p.row_blocks;
    const int nch = want < nseg ? (want < 1 ? 1 : want) : nseg;
    int s0 = 0;
    for (int k = 0; k < nch; k++) {
        int s1k = nseg;
        if (k + 1 < nch) {
            const int left = nnz - p.segs[s0].first;
            const int target = p.segs[s0].first + (left + (nch - k) - 1) / (nch - k);
            s1k = s0 + 1;
            while (s1k < nseg - (nch - 1 - k) && p.segs[s1k].first < target) s1k++;
        }
        hb_pvechunk c;
        c.first = s0, c.count = s1k - s0;
        p.chunks.push_back(c);
        s0 = s1k;
    }
    return p;
}
