// hb_impute.hip — ssbrm()'s imputation of the non-genotyped individuals' genotypes, Mn = solve(A^-1_nn, -A^-1_ng M) with Jn beside it
// (R/ssbayes.r:295-307), on the device without a factor: conjugate gradients with the Jacobi preconditioner, all right-hand sides of a block
// advancing in lockstep. A unit of its own: it shares hb_wave.hpp's types with the others and nothing else. DESIGN.md §19;
// tests/impute_restatement.py states the same algorithm in numpy.
//
// Layout: the lane is the right-hand side. A block vector (x, r, p, Ap, b) is q rows of W doubles, W a multiple of 64 (hb_imputeplan.hpp): a
// wave owns a row, each lane one marker column of it, and grid.y walks the W / 64 column groups. A^-1_nn is symmetric, so its row i is its CSC
// column i — one contiguous run of indices and values, wave-uniform (scalar loads) — and every stored entry costs one coalesced 512-byte read
// of a row of p.
//
// One iteration = three launches, the kernel boundary being the only grid-wide synchronisation:
//   k_imp_product  Ap = A p, and each workgroup's per-column partial sums of p . Ap
//   k_imp_step1    every workgroup re-adds those partials -> pAp, and those of r . z; alpha = rz / pAp; x += alpha p; r -= alpha Ap; leaves the
//                  partials of r . r and of r . z (z = D^-1 r is never stored)
//   k_imp_step2    the stop test ||r|| <= tol ||b|| per column; a column that passes is FROZEN: done[column] is set and no kernel touches its
//                  x, r or p again; the others: beta = rz_new / rz, p = z + beta p. When every column of a group of 64 is frozen the group's
//                  stop word is set, and a kernel enqueued for a later iteration returns at once.
// No floating-point atomic: every per-column sum over the rows is formed over the partition of hb_impute_partition() — a function of q alone —
// in one fixed order, and a lane's arithmetic reads nothing of another lane's. So two runs agree bit for bit, and a column's result has the
// same bits alone, in any block, at any lane. The unit is built with -ffp-contract=off: its expressions round as written.
//
// done[c] and the stop word hold 1 + the number of iterations after which the column / group needs no more (0: live), so the words a launch
// of iteration `it` writes (it + 2) do not count for that launch: no workgroup's decision depends on a word another workgroup of the same
// launch writes. The host enqueues iterations in chunks and looks at the stop words once per chunk (IMP_LOOK).
#include "hb_internal.hpp"
#include "hb_imputeplan.hpp"
#include "hb_wave.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {
constexpr int IMP_T = IMP_WAVES * 64; // threads per workgroup of the solver's kernels
constexpr int IMP_LOOK = 32;          // iterations enqueued between two looks at the stop words

typedef double imp_red[IMP_WAVES][64];

__device__ __forceinline__ bool imp_stopped(const int *stopg, int it)
{
    if (!stopg) return false;
    const int s = stopg[blockIdx.y];
    return s != 0 && it >= s - 1;
}
__device__ __forceinline__ bool imp_frozen(int done, int it) { return done != 0 && it >= done - 1; }

// N sums at once, each of n partials of this lane's column: in.p[a][k][col], k = 0 .. n - 1. Wave w adds the partials w, w + IMP_WAVES, ... in
// ascending order, the waves' sums are added in wave order — the same order in every workgroup that forms the sum; the results in every
// thread. The loads of eight turns (of all N sums) are issued before the first of them is added: the adds stay in order, the round trips to
// L2 do not queue up behind each other.
template <int N> struct imp_ptrs {
    const double *p[N];
};
template <int N>
__device__ __forceinline__ void imp_colsums(const imp_ptrs<N> in, int n, int W, int col, int wave, int lane, imp_red (&red)[N], double (&out)[N])
{
    double s[N];
#pragma unroll
    for (int a = 0; a < N; a++) s[a] = 0.0;
    for (int k = wave; k < n; k += 8 * IMP_WAVES) {
        double v[N][8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int ku = min(k + u * IMP_WAVES, n - 1); // (a turn past the end reads the last partial and adds nothing)
#pragma unroll
            for (int a = 0; a < N; a++) v[a][u] = in.p[a][(size_t)ku * W + col];
        }
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (k + u * IMP_WAVES < n) {
#pragma unroll
                for (int a = 0; a < N; a++) s[a] += v[a][u];
            }
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < N; a++) red[a][wave][lane] = s[a];
    __syncthreads();
#pragma unroll
    for (int a = 0; a < N; a++) {
        double t = red[a][0][lane];
#pragma unroll
        for (int w = 1; w < IMP_WAVES; w++) t += red[a][w][lane];
        out[a] = t;
    }
}

// the workgroup's partial of this lane's column: the waves' sums added in wave order
__device__ __forceinline__ void imp_put(double c, double *__restrict__ parts, int W, int col, int wave, int lane, imp_red &red)
{
    __syncthreads();
    red[wave][lane] = c;
    __syncthreads();
    if (wave == 0) {
        double t = red[0][lane];
#pragma unroll
        for (int w = 1; w < IMP_WAVES; w++) t += red[w][lane];
        parts[(size_t)blockIdx.x * W + col] = t;
    }
}

#define IMP_GEOM                                                               \
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   \
    const int lane = threadIdx.x & 63;                                          \
    const int col = blockIdx.y * 64 + lane;                                     \
    const int row0 = blockIdx.x * rows, row1 = min(row0 + rows, q);

// dst (nc x nr, row stride ldd) = the transpose of src (nr x nc, row stride lds): the uploaded column-major chunk of M into the block layout,
// and x back into a column-major chunk. 32 x 32 tiles, 256 threads.
__global__ __launch_bounds__(256) void k_imp_transpose(const double *__restrict__ src, size_t lds, double *__restrict__ dst, size_t ldd, int nr, int nc)
{
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int yy = ty; yy < 32; yy += 8) {
        const int r = blockIdx.y * 32 + yy, c = blockIdx.x * 32 + tx;
        if (r < nr && c < nc) tile[yy][tx] = src[(size_t)r * lds + c];
    }
    __syncthreads();
    for (int yy = ty; yy < 32; yy += 8) {
        const int c = blockIdx.x * 32 + yy, r = blockIdx.y * 32 + tx;
        if (r < nr && c < nc) dst[(size_t)c * ldd + r] = tile[tx][yy];
    }
}

// b = -A_ng M over the CSR rows (Mt: n_g rows of W); x = 0, r = b, p = z = D^-1 b; the partials of b . b and of r . z (half 0)
__global__ __launch_bounds__(IMP_T) void k_imp_init(const int64_t *__restrict__ gp, const int32_t *__restrict__ gi, const double *__restrict__ gv, int q,
                                                    int W, int rows, const double *__restrict__ Mt, const double *__restrict__ dinv,
                                                    double *__restrict__ b, double *__restrict__ x, double *__restrict__ r, double *__restrict__ p,
                                                    double *__restrict__ bb_parts, double *__restrict__ rz_parts)
{
    __shared__ imp_red red;
    IMP_GEOM
    double cbb = 0.0, crz = 0.0;
    for (int i = row0 + wave; i < row1; i += IMP_WAVES) {
        const int64_t e1 = gp[i + 1];
        double s = 0.0;
#pragma unroll 4
        for (int64_t e = gp[i]; e < e1; e++) s += gv[e] * Mt[(size_t)gi[e] * W + col];
        const double bi = -s, zi = dinv[i] * bi;
        const size_t at = (size_t)i * W + col;
        b[at] = bi;
        x[at] = 0.0;
        r[at] = bi;
        p[at] = zi;
        cbb += bi * bi;
        crz += bi * zi;
    }
    imp_put(cbb, bb_parts, W, col, wave, lane, red);
    imp_put(crz, rz_parts, W, col, wave, lane, red);
}

// one workgroup per column group: bb[c] = ||b_c||^2; a column with b = 0 stops before the first iteration with x = 0 (no 0 / 0 is formed)
__global__ __launch_bounds__(IMP_T) void k_imp_start(const double *__restrict__ bb_parts, int P, int W, double tol2, double *__restrict__ bb,
                                                     int *__restrict__ done, int *__restrict__ stopg)
{
    __shared__ imp_red red[1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = blockIdx.y * 64 + lane;
    double sum[1];
    imp_colsums<1>({{bb_parts}}, P, W, col, wave, lane, red, sum);
    const double s = sum[0];
    const bool stop = s <= tol2 * s; // (r = b)
    if (wave == 0) {
        bb[col] = s;
        done[col] = stop ? 1 : 0;
        if (__all(stop) && lane == 0) stopg[blockIdx.y] = 1;
    }
}

// Ap = A p over the rows of the symmetric CSC, a wave per row; parts[workgroup][c] = the run's sum of p[i][c] Ap[i][c]
__global__ __launch_bounds__(IMP_T) void k_imp_product(const int64_t *__restrict__ cp, const int32_t *__restrict__ ri, const double *__restrict__ va, int q,
                                                       int W, int rows, const double *__restrict__ p, double *__restrict__ ap,
                                                       double *__restrict__ parts, const int *stopg, int it)
{
    __shared__ imp_red red;
    if (imp_stopped(stopg, it)) return; // (uniform)
    IMP_GEOM
    double c = 0.0;
    for (int i = row0 + wave; i < row1; i += IMP_WAVES) {
        const int64_t e1 = cp[i + 1];
        double s = 0.0;
#pragma unroll 4
        for (int64_t e = cp[i]; e < e1; e++) s += va[e] * p[(size_t)ri[e] * W + col];
        const size_t at = (size_t)i * W + col;
        ap[at] = s;
        c += p[at] * s;
    }
    imp_put(c, parts, W, col, wave, lane, red);
}

// rz: two halves of P x W partials of r . z, the half of iteration `it`'s parity holds the current one
__global__ __launch_bounds__(IMP_T) void k_imp_step1(int it, int q, int W, int rows, int P, const double *__restrict__ pap_parts, double *__restrict__ rz_parts,
                                                     double *__restrict__ rr_parts, const double *__restrict__ p, const double *__restrict__ ap,
                                                     double *__restrict__ x, double *__restrict__ r, const double *__restrict__ dinv,
                                                     const int *done, const int *stopg, int *__restrict__ errg)
{
    __shared__ imp_red red[2];
    if (imp_stopped(stopg, it)) return; // (uniform)
    IMP_GEOM
    const size_t half = (size_t)P * W;
    double sum[2];
    imp_colsums<2>({{pap_parts, rz_parts + (size_t)(it & 1) * half}}, P, W, col, wave, lane, red, sum);
    const double pAp = sum[0], rz = sum[1];
    const bool live = !imp_frozen(done[col], it);
    const bool bad = live && !(pAp > 0.0); // not positive definite (or not a number)
    if (bad && blockIdx.x == 0 && wave == 0) errg[blockIdx.y] = it + 1;
    double crr = 0.0, crz = 0.0;
    if (live && !bad) {
        const double alpha = rz / pAp;
        for (int i = row0 + wave; i < row1; i += IMP_WAVES) {
            const size_t at = (size_t)i * W + col;
            x[at] = x[at] + alpha * p[at];
            const double ri_ = r[at] - alpha * ap[at];
            r[at] = ri_;
            crr += ri_ * ri_;
            crz += ri_ * (dinv[i] * ri_);
        }
    }
    imp_put(crr, rr_parts, W, col, wave, lane, red[0]);
    imp_put(crz, rz_parts + (size_t)((it + 1) & 1) * half, W, col, wave, lane, red[1]);
}

__global__ __launch_bounds__(IMP_T) void k_imp_step2(int it, int q, int W, int rows, int P, const double *__restrict__ rr_parts,
                                                     const double *__restrict__ rz_parts, const double *__restrict__ bb, double tol2,
                                                     const double *__restrict__ r, double *__restrict__ p, const double *__restrict__ dinv, int *done,
                                                     int *stopg)
{
    __shared__ imp_red red[3];
    if (imp_stopped(stopg, it)) return; // (uniform; a word written by this very launch is it + 2 and does not count)
    IMP_GEOM
    const size_t half = (size_t)P * W;
    double sum[3];
    imp_colsums<3>({{rr_parts, rz_parts + (size_t)((it + 1) & 1) * half, rz_parts + (size_t)(it & 1) * half}}, P, W, col, wave, lane, red, sum);
    const double rr = sum[0], rz_new = sum[1], rz = sum[2];
    const bool frozen = imp_frozen(done[col], it);
    const bool stop = !frozen && rr <= tol2 * bb[col];
    if (blockIdx.x == 0 && wave == 0) {
        if (stop) done[col] = it + 2;
        if (__all(frozen || stop) && lane == 0) stopg[blockIdx.y] = it + 2;
    }
    if (frozen || stop) return; // (this lane)
    const double beta = rz_new / rz;
    for (int i = row0 + wave; i < row1; i += IMP_WAVES) {
        const size_t at = (size_t)i * W + col;
        const double ri_ = r[at];
        p[at] = dinv[i] * ri_ + beta * p[at];
    }
}

// the partials of ||b - A x||^2 (ap = A x)
__global__ __launch_bounds__(IMP_T) void k_imp_resid(int q, int W, int rows, const double *__restrict__ b, const double *__restrict__ ap,
                                                     double *__restrict__ parts)
{
    __shared__ imp_red red;
    IMP_GEOM
    double c = 0.0;
    for (int i = row0 + wave; i < row1; i += IMP_WAVES) {
        const size_t at = (size_t)i * W + col;
        const double d = b[at] - ap[at];
        c += d * d;
    }
    imp_put(c, parts, W, col, wave, lane, red);
}

// one workgroup per column group: out[c] = the sum of its partials
__global__ __launch_bounds__(IMP_T) void k_imp_fin(const double *__restrict__ parts, int P, int W, double *__restrict__ out)
{
    __shared__ imp_red red[1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = blockIdx.y * 64 + lane;
    double sum[1];
    imp_colsums<1>({{parts}}, P, W, col, wave, lane, red, sum);
    if (wave == 0) out[col] = sum[0];
}
} // namespace

// the matrices of one system on the device, and the stream its solves run on
struct hb_impute {
    int device = 0;
    int32_t q = 0, n_g = 0;
    int64_t nnz_nn = 0, nnz_ng = 0;
    hipStream_t stream = nullptr;
    hb_bufs mem;
    int64_t *cp = nullptr, *gp = nullptr;
    int32_t *ri = nullptr, *gi = nullptr;
    double *va = nullptr, *gv = nullptr, *dinv = nullptr;
    ~hb_impute()
    {
        if (stream) (void)hipStreamSynchronize(stream);
        mem.clear();
        if (stream) (void)hipStreamDestroy(stream);
    }
};

extern "C" int hb_impute_create(int32_t q, const int64_t *nn_indptr, const int32_t *nn_indices, const double *nn_data, int32_t ng_rows, int32_t n_g,
                                const int64_t *ng_indptr, const int32_t *ng_indices, const double *ng_data, int32_t device, hb_impute **out)
{
    if (!out) return hb_fail(HB_ERR_INVALID, "hb_impute_create: null argument");
    *out = nullptr;
    const std::string bad = hb_impute_check_args(q, nn_indptr, nn_indices, nn_data, ng_rows, n_g, ng_indptr, ng_indices, ng_data);
    if (!bad.empty()) return hb_fail(HB_ERR_INVALID, "hb_impute_create: " + bad);
    if (hb_device_count() <= 0) return hb_fail(HB_ERR_NO_DEVICE, "no HIP device available: the hibayes GPU engine has no CPU fallback");
    if (device < 0 || device >= hb_device_count()) return hb_fail(HB_ERR_INVALID, "hb_impute_create: no such device");
    HB_HIP(hipSetDevice(device));
    hb_impute *h = new hb_impute;
    struct guard {
        hb_impute *h;
        ~guard() { delete h; }
    } g{h};
    h->device = device;
    h->q = q;
    h->n_g = n_g;
    h->nnz_nn = nn_indptr[q];
    h->nnz_ng = ng_indptr[q];
    HB_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    std::vector<double> dinv(q);
    for (int32_t i = 0; i < q; i++) {
        const int32_t *b = nn_indices + nn_indptr[i], *e = nn_indices + nn_indptr[i + 1];
        dinv[i] = 1.0 / nn_data[std::lower_bound(b, e, i) - nn_indices];
    }
    HB_TRY(h->mem.get(&h->cp, (size_t)q + 1));
    HB_TRY(h->mem.get(&h->ri, (size_t)h->nnz_nn));
    HB_TRY(h->mem.get(&h->va, (size_t)h->nnz_nn));
    HB_TRY(h->mem.get(&h->gp, (size_t)q + 1));
    HB_TRY(h->mem.get(&h->gi, (size_t)h->nnz_ng));
    HB_TRY(h->mem.get(&h->gv, (size_t)h->nnz_ng));
    HB_TRY(h->mem.get(&h->dinv, (size_t)q));
    HB_HIP(hipMemcpyAsync(h->cp, nn_indptr, sizeof(int64_t) * ((size_t)q + 1), hipMemcpyHostToDevice, h->stream));
    HB_HIP(hipMemcpyAsync(h->ri, nn_indices, sizeof(int32_t) * (size_t)h->nnz_nn, hipMemcpyHostToDevice, h->stream));
    HB_HIP(hipMemcpyAsync(h->va, nn_data, sizeof(double) * (size_t)h->nnz_nn, hipMemcpyHostToDevice, h->stream));
    HB_HIP(hipMemcpyAsync(h->gp, ng_indptr, sizeof(int64_t) * ((size_t)q + 1), hipMemcpyHostToDevice, h->stream));
    HB_HIP(hipMemcpyAsync(h->gi, ng_indices, sizeof(int32_t) * (size_t)h->nnz_ng, hipMemcpyHostToDevice, h->stream));
    HB_HIP(hipMemcpyAsync(h->gv, ng_data, sizeof(double) * (size_t)h->nnz_ng, hipMemcpyHostToDevice, h->stream));
    HB_HIP(hipMemcpyAsync(h->dinv, dinv.data(), sizeof(double) * (size_t)q, hipMemcpyHostToDevice, h->stream));
    HB_HIP(hipStreamSynchronize(h->stream));
    g.h = nullptr;
    *out = h;
    return HB_OK;
}

extern "C" void hb_impute_destroy(hb_impute *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}

extern "C" int hb_impute_solve(hb_impute *h, const double *M, int64_t ld, int32_t ncols, double tol, int32_t max_iter, double *Mn, int64_t ld_out,
                               hb_impute_stats *stats)
{
    if (!(tol > 0.0 && tol < 1.0)) return hb_fail(HB_ERR_INVALID, "hb_impute_solve: tol must lie inside (0, 1)");
    if (max_iter < 1) return hb_fail(HB_ERR_INVALID, "hb_impute_solve: max_iter must be at least 1");
    if (!h) return hb_fail(HB_ERR_INVALID, "hb_impute_solve: null handle");
    if (!M || !Mn || ncols < 1 || ld < h->n_g || ld_out < h->q) return hb_fail(HB_ERR_INVALID, "hb_impute_solve: M (n_g x columns, ld >= n_g) and the output (q x columns, ld >= q) are required");
    const auto t0 = hb_clk::now();
    const int q = h->q, ng = h->n_g;
    HB_HIP(hipSetDevice(h->device));
    size_t free_b = 0, total_b = 0;
    HB_HIP(hipMemGetInfo(&free_b, &total_b));
    const hb_impute_plan pl = hb_impute_plan_of(q, h->nnz_nn, ng, h->nnz_ng, ncols, (int64_t)free_b);
    if (!pl.ok) return hb_fail(HB_ERR_UNSUPPORTED, pl.why);
    const int W = pl.width, G = pl.groups, P = pl.parts, rows = pl.rows_per_part;
    hipStream_t s = h->stream;
    hb_bufs mem;
    struct sync_first { // the stream is drained before the buffers go, on every way out
        hipStream_t s;
        ~sync_first() { (void)hipStreamSynchronize(s); }
    };
    const size_t block = (size_t)q * W, half = (size_t)P * W;
    double *d_min, *d_mt, *d_b, *d_x, *d_r, *d_p, *d_ap, *d_pap, *d_rr, *d_rz, *d_bb, *d_res;
    int *d_done, *d_stopg, *d_errg, *h_words;
    double *h_cols;
    HB_TRY(mem.get(&d_min, (size_t)ng * W));
    HB_TRY(mem.get(&d_mt, (size_t)ng * W));
    HB_TRY(mem.get(&d_b, block));
    HB_TRY(mem.get(&d_x, block));
    HB_TRY(mem.get(&d_r, block));
    HB_TRY(mem.get(&d_p, block));
    HB_TRY(mem.get(&d_ap, block));
    HB_TRY(mem.get(&d_pap, half));
    HB_TRY(mem.get(&d_rr, half));
    HB_TRY(mem.get(&d_rz, 2 * half));
    HB_TRY(mem.get(&d_bb, (size_t)W));
    HB_TRY(mem.get(&d_res, (size_t)W));
    HB_TRY(mem.get(&d_done, (size_t)W));
    HB_TRY(mem.get(&d_stopg, (size_t)2 * G)); // the stop words, then the error words
    d_errg = d_stopg + G;
    HB_TRY(mem.pin(&h_words, (size_t)2 * G + W));
    HB_TRY(mem.pin(&h_cols, (size_t)2 * W));
    sync_first drain{s};
    const dim3 grid((unsigned)P, (unsigned)G), one(1, (unsigned)G), thr(IMP_T);
    const double tol2 = tol * tol;
    const bool profile = getenv("HB_IMPUTE_PROFILE") != nullptr; // time the product kernel alone after each block's solve (tools/epsl_timing.py)
    hb_impute_stats st{};
    st.width = W;
    st.parts = P;
    st.cached = pl.cached;
    st.product_bytes = (h->nnz_nn + (int64_t)q) * W * 8 + h->nnz_nn * 12 + ((int64_t)q + 1) * 8; // gathered rows of p, Ap written, the matrix
    auto transpose = [&](const double *src, size_t lds, double *dst, size_t ldd, int nr, int nc) {
        hipLaunchKernelGGL(k_imp_transpose, dim3((unsigned)((nc + 31) / 32), (unsigned)((nr + 31) / 32)), dim3(256), 0, s, src, lds, dst, ldd, nr, nc);
    };
    for (int c0 = 0; c0 < ncols; c0 += W) {
        const int k = std::min(W, ncols - c0);
        // ---- the chunk of M into the block layout; columns k .. W - 1 are zero columns: they stop before the first iteration ----
        HB_HIP(hipMemsetAsync(d_mt, 0, sizeof(double) * (size_t)ng * W, s));
        HB_HIP(hipMemsetAsync(d_stopg, 0, sizeof(int) * 2 * G, s));
        HB_HIP(hipMemcpy2DAsync(d_min, sizeof(double) * ng, M + (size_t)c0 * (size_t)ld, sizeof(double) * ld, sizeof(double) * ng, k, hipMemcpyHostToDevice, s));
        transpose(d_min, (size_t)ng, d_mt, (size_t)W, k, ng);
        hipLaunchKernelGGL(k_imp_init, grid, thr, 0, s, h->gp, h->gi, h->gv, q, W, rows, d_mt, h->dinv, d_b, d_x, d_r, d_p, d_pap, d_rz);
        hipLaunchKernelGGL(k_imp_start, one, thr, 0, s, d_pap, P, W, tol2, d_bb, d_done, d_stopg);
        HB_HIP(hipGetLastError());
        // ---- iterations in chunks, one look at the stop words per chunk ----
        int ran = 0;
        bool all = false;
        for (int it0 = 0; it0 < max_iter && !all;) {
            const int c = std::min(IMP_LOOK, max_iter - it0);
            for (int it = it0; it < it0 + c; it++) {
                hipLaunchKernelGGL(k_imp_product, grid, thr, 0, s, h->cp, h->ri, h->va, q, W, rows, d_p, d_ap, d_pap, d_stopg, it);
                hipLaunchKernelGGL(k_imp_step1, grid, thr, 0, s, it, q, W, rows, P, d_pap, d_rz, d_rr, d_p, d_ap, d_x, d_r, h->dinv, d_done, d_stopg, d_errg);
                hipLaunchKernelGGL(k_imp_step2, grid, thr, 0, s, it, q, W, rows, P, d_rr, d_rz, d_bb, tol2, d_r, d_p, h->dinv, d_done, d_stopg);
            }
            HB_HIP(hipGetLastError());
            HB_HIP(hipMemcpyAsync(h_words, d_stopg, sizeof(int) * 2 * G, hipMemcpyDeviceToHost, s));
            HB_HIP(hipStreamSynchronize(s));
            it0 += c;
            all = true;
            ran = 0;
            for (int g = 0; g < G; g++) {
                if (h_words[G + g]) {
                    char buf[200];
                    snprintf(buf, sizeof(buf), "hb_impute_solve: p'Ap <= 0 at iteration %d (columns %d..%d): A_nn is not positive definite", h_words[G + g] - 1,
                             c0 + 64 * g, c0 + 64 * g + 63);
                    return hb_fail(HB_ERR_INVALID, buf);
                }
                all = all && h_words[g] != 0;
                ran = std::max(ran, h_words[g] ? h_words[g] - 1 : it0);
            }
            st.looks++;
        }
        if (!all) {
            HB_HIP(hipMemcpyAsync(h_words + 2 * G, d_done, sizeof(int) * W, hipMemcpyDeviceToHost, s));
            HB_HIP(hipStreamSynchronize(s));
            int live = 0;
            for (int c = 0; c < k; c++) live += h_words[2 * G + c] == 0;
            char buf[200];
            snprintf(buf, sizeof(buf), "hb_impute_solve: %d of %d columns (from column %d) did not converge to tol = %g within %d iterations", live, k, c0, tol,
                     max_iter);
            return hb_fail(HB_ERR_INVALID, buf);
        }
        st.iterations = std::max(st.iterations, ran);
        if (profile) { // the product alone, on the p the solve left
            hipEvent_t e0, e1;
            HB_HIP(hipEventCreate(&e0));
            HB_HIP(hipEventCreate(&e1));
            const int reps = 10;
            hipLaunchKernelGGL(k_imp_product, grid, thr, 0, s, h->cp, h->ri, h->va, q, W, rows, d_p, d_ap, d_pap, (const int *)nullptr, 0);
            HB_HIP(hipEventRecord(e0, s));
            for (int rep = 0; rep < reps; rep++)
                hipLaunchKernelGGL(k_imp_product, grid, thr, 0, s, h->cp, h->ri, h->va, q, W, rows, d_p, d_ap, d_pap, (const int *)nullptr, 0);
            HB_HIP(hipEventRecord(e1, s));
            HB_HIP(hipEventSynchronize(e1));
            float ms = 0.f;
            HB_HIP(hipEventElapsedTime(&ms, e0, e1));
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
            st.product_seconds = 1e-3 * ms / reps;
        }
        // ---- one more product: the true residual b - A x, per column ----
        hipLaunchKernelGGL(k_imp_product, grid, thr, 0, s, h->cp, h->ri, h->va, q, W, rows, d_x, d_ap, d_pap, (const int *)nullptr, 0);
        hipLaunchKernelGGL(k_imp_resid, grid, thr, 0, s, q, W, rows, d_b, d_ap, d_pap);
        hipLaunchKernelGGL(k_imp_fin, one, thr, 0, s, d_pap, P, W, d_res);
        transpose(d_x, (size_t)W, d_ap, (size_t)q, q, k); // (Ap is free now: the column-major result)
        HB_HIP(hipGetLastError());
        HB_HIP(hipMemcpyAsync(h_cols, d_res, sizeof(double) * W, hipMemcpyDeviceToHost, s));
        HB_HIP(hipMemcpyAsync(h_cols + W, d_bb, sizeof(double) * W, hipMemcpyDeviceToHost, s));
        HB_HIP(hipMemcpy2DAsync(Mn + (size_t)c0 * (size_t)ld_out, sizeof(double) * ld_out, d_ap, sizeof(double) * q, sizeof(double) * q, k, hipMemcpyDeviceToHost, s));
        HB_HIP(hipStreamSynchronize(s));
        for (int c = 0; c < k; c++)
            if (h_cols[W + c] > 0.0) st.max_residual = std::max(st.max_residual, std::sqrt(h_cols[c] / h_cols[W + c]));
        st.blocks++;
    }
    st.seconds = hb_since(t0);
    if (stats) *stats = st;
    return HB_OK;
}
