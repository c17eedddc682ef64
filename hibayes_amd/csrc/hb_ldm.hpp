// hb_ldm.hpp — the LD-matrix handle (hb_ldm_build, hb_ldmat.hip) as the units that use it see it: hb_ldmat.hip owns it,
// hb_sbayes.hip reads its diagonal and adopts its dense device copy (hb_sbayes_run_ldm). hb_kernels.hip does not include this.
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
};

// true once genotypes were uploaded to / generated on the context (hb_ctx.hip keeps the list: hb_ctx itself is laid out in
// hb_internal.hpp, which the chain kernels' unit includes and this feature leaves alone)
bool hb_ctx_has_genotypes(const hb_ctx *c);
// the dense device copy, made from the host copy if the build did not keep one
int hb_ldm_device_dense(hb_ldm *l, const double **out);
