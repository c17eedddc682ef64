// hb_ldm.hpp — the LD-matrix handle (hb_ldm_build, hb_ldmat.hip) as the units that use it see it: hb_ldmat.hip owns it,
// hb_sbayes.hip reads its diagonal and adopts its dense device copy (hb_sbayes_run_ldm) or its device CSC (hb_sbayes_run_sparse). hb_kernels.hip does not include this.
#pragma once
#include "hb_internal.hpp"

struct hb_ldm {
    int device = 0;
    int m = 0, kind = HB_LDM_KIND_DENSE, n_strips = 0;
    int64_t nnz = 0;
    double seconds = 0, t_stats = 0, t_strips = 0, t_compact = 0, t_xfer = 0;
    // genome-wide dense: the matrix itself, pinned, m x m column-major
    double *h_dense = nullptr;
    // every other kind: the compacted strips as they left the device (pinned, grown by doubling), column j's row-sorted
    // entries at [col_off[j], col_off[j] + col_cnt[j]) — the strips come in the build's column order, hb_ldm_download_csc
    // lays them out in marker order
    int32_t *h_idx = nullptr;
    double *h_val = nullptr;
    int64_t h_cap = 0, h_used = 0;
    std::vector<int64_t> col_off;
    std::vector<int32_t> col_cnt;
    std::vector<double> diag; // ldm[j][j] (0 where the sparse matrix stores nothing): what SBayesD() reads first (src/SBayesD.cpp:95-99)
    double *d_dense = nullptr; // m x m, leading dimension m, zeros where nothing is stored; nullptr: not held (hb_ldm_device_dense makes it)
    // the device CSC in marker order, for the sparse sampler (hb_ldm_device_csc makes it; nullptr: not held)
    int64_t *d_cp = nullptr;   // [m + 1] column pointers
    int32_t *d_ri = nullptr;   // [csc_nnz] row indices, sorted inside a column
    double *d_va = nullptr;    // [csc_nnz] values
    int32_t *d_cnt = nullptr;  // [m] stored entries per column (varediff, src/SBayesS.cpp:131-141); m for the dense kind
    int64_t *d_run = nullptr;  // [m] first entry of column j inside the rows of j's own group of HB_LDM_GS markers ...
    int32_t *d_runn = nullptr; // [m] ... and how many there are (contiguous: rows are sorted)
    int64_t csc_nnz = 0;
    std::vector<int32_t> grp_lo, grp_hi; // per group: the rows [lo, hi) its columns touch (lo == hi: none)
    hb_bufs mem; // every pinned and device buffer above
};

#define HB_LDM_GS 512 // markers per group of the sparse sweep (SS_GS, hb_sbayes_sparse.hpp)
struct hb_ldm_csc {
    int64_t nnz;
    const int64_t *cp, *run;
    const int32_t *ri, *cnt, *runn;
    const double *va;
    const int32_t *grp_lo, *grp_hi; // host
};

// true once genotypes were uploaded to / generated on the context (hb_ctx.hip keeps the list: hb_ctx itself is laid out in
// hb_internal.hpp, which the chain kernels' unit includes and this feature leaves alone)
bool hb_ctx_has_genotypes(const hb_ctx *c);
// the dense device copy, made from the host copy if the build did not keep one
int hb_ldm_device_dense(hb_ldm *l, const double **out);
// the device CSC, made from the host copy on first use: the stored entries of the strips, or the non-zero entries of the
// genome-wide dense matrix. Nothing m x m is allocated on the device.
int hb_ldm_device_csc(hb_ldm *l, hb_ldm_csc *out);
