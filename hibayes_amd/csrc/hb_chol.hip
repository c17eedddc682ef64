// hb_chol.hip — the inverse of a symmetric positive definite matrix on the device: what make_grm(inverse = TRUE) asks of solve() (reference
// src/rm.cpp:39-42 -> solver_chol(), src/solver.cpp:159-202): LAPACK dpotrf('L'), dpotri('L') and the mirror, on an n x n column-major fp64 matrix
// (DESIGN.md §20). A unit of its own: it shares hb_mma.hpp's fp64 matrix-core wrapper and triangle decode with the other dense units, nothing else.
// hb_cholplan.hpp decides the panel width NB = 64, the work buffer and every panel's launch sizes.
//
// Stage 1, dpotrf: right-looking, a panel of NB columns at a time (k0, k1 = k0 + NB):
//     k_chol_diag    one workgroup: the NB x NB diagonal block factored in LDS, column by column. A pivot that is not > 0 (a NaN included)
//                    stops it: info = the 1-based order of that minor goes to a device word, and every later kernel of the call returns at once
//     k_chol_panel   L21 = A21 L11^-T by substitution, a thread per row: its 64 entries stay in registers, L11 in LDS is read at wave-uniform addresses
//     k_chol_trail   A22 -= L21 L21' on the matrix cores (v_mfma_f64_16x16x4_f64): 64 x 64 tiles bi >= bj of the lower triangle, entries j <= i only
// Stage 2, dtrtri('L', 'N'), in place:
//     k_chol_dinv    every diagonal block inverted in LDS by forward substitution on the identity, one workgroup each, one launch
//     then per block of columns from the last but one to the first, with X22 the inverse of the trailing triangle already in place:
//     k_chol_trmm    P = X22 L21 into the panel buffer (a triangular GEMM: a row tile sums over k up to its own rows)
//     k_chol_tscale  X21 = -P X11 back into the matrix
//     — on two levels: first inside the diagonal super-blocks of 256, all of them in the same launches, block columns of 64; then the super-block
//     columns, 256 wide: four times the workgroups per launch and a quarter of the launches that block columns of 64 alone would give
// Stage 3, dlauum: X = L^-T L^-1 out of place, k_chol_lauum: the tile (bi, bj), bi >= bj, sums the k-blocks >= bi and stores each entry at (i, j)
//     and at (j, i) from the same register, so X equals its transpose bit for bit.
// The strict upper triangle of the input is never read and, by stages 1 and 2, never written. No floating-point atomic and one summation order
// that depends on n alone: two runs agree bit for bit. No kernel waits for another workgroup: a panel depends on the one before through stream
// order only. None uses scratch (hb_chol.res.txt; tests/test_chol_host.py).
#include "hb_internal.hpp"
#include "hb_mma.hpp"
#include "hb_cholplan.hpp"
#include <cmath>
#include <cstdio>

namespace {

constexpr int NB = HB_CHOL_NB, SB = HB_CHOL_SB;
static_assert(NB == 64, "the tiles below are 64 x 64: four waves of 32 x 32");
static_assert(SB % NB == 0 && SB > NB, "a super-block of the factor's inverse is a whole number of panels");

// acc += sum over k in [kbeg, kend), four at a time, of fa(ii, k) fb(k, jj): ii, jj in [0, 32) are the wave's rows and columns. Afterwards register r of
// acc[a][b] holds the entry of row mma_f64_col(a, lane) and column mma_f64_row(b, r, lane): the rows run along the lanes, contiguous in memory.
template <class FA, class FB> __device__ __forceinline__ void tile_mma(v4d (&acc)[2][2], int kbeg, int kend, int lane, FA fa, FB fb)
{
    const int lr = lane & 15, q = lane >> 4;
    for (int kk = kbeg; kk < kend; kk += 4) {
        const int k = kk + q;
        double ya[2], xb[2];
#pragma unroll
        for (int a = 0; a < 2; a++) {
            ya[a] = fa(16 * a + lr, k);
            xb[a] = fb(k, 16 * a + lr);
        }
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++) acc[a][b] = mfma_f64(xb[b], ya[a], acc[a][b]);
    }
}

// A[i][i] += lambda
__global__ __launch_bounds__(256) void k_chol_shift(double *__restrict__ A, int64_t lda, int n, double lambda)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) A[(int64_t)i * lda + i] += lambda;
}

// W <- the lower triangle of A + lambda I (blockIdx.x: the column, blockIdx.y: 256 of its rows); the rest of W is never read
__global__ __launch_bounds__(256) void k_chol_copy(const double *__restrict__ A, int64_t lda, int n, double *__restrict__ W, int64_t ldw, double lambda, int shift)
{
    const int j = blockIdx.x, i = blockIdx.y * 256 + threadIdx.x;
    if (i >= n || i < j) return;
    double v = A[(int64_t)j * lda + i];
    if (shift && i == j) v += lambda;
    W[(int64_t)j * ldw + i] = v;
}

// the diagonal block [k0, k0 + w)^2 factored in LDS (padded to 64 with the identity). Right-looking: per column the pivot's root, the column scaled,
// the block's remaining columns updated. Thread t owns row t & 63 and every fourth column from t >> 6.
__global__ __launch_bounds__(256) void k_chol_diag(double *__restrict__ A, int64_t lda, int k0, int w, int *__restrict__ info)
{
    __shared__ double s[NB][NB + 1];
    if (*info) return;
    const int t = threadIdx.x, i = t & 63, g = t >> 6;
    double *Ab = A + (int64_t)k0 * lda + k0;
    for (int c = g; c < NB; c += 4) s[i][c] = (i < w && c <= i) ? Ab[(int64_t)c * lda + i] : (i == c ? 1.0 : 0.0);
    __syncthreads();
    for (int j = 0; j < w; j++) {
        const double ajj = s[j][j];
        if (!(ajj > 0.0)) { // (the same value in every thread: they all leave)
            if (t == 0) *info = k0 + j + 1;
            break;
        }
        __syncthreads(); // everybody has the pivot
        const double d = sqrt(ajj);
        if (g == 0) {
            if (i > j) s[i][j] /= d;
            if (i == j) s[j][j] = d;
        }
        __syncthreads();
        if (i > j) {
            const double lij = s[i][j];
            for (int c = j + 1 + g; c <= i; c += 4) s[i][c] = fma(-lij, s[c][j], s[i][c]);
        }
        __syncthreads();
    }
    __syncthreads();
    for (int c = g; c < NB; c += 4)
        if (i < w && c <= i) Ab[(int64_t)c * lda + i] = s[i][c];
}

// L21 = A21 L11^-T for the rows below a full diagonal block: x L11' = b per row, forward over the 64 columns, the row in registers (everything unrolled:
// no indexed register array). L11 is staged in LDS and read at addresses that do not depend on the lane (broadcasts).
__global__ __launch_bounds__(64) void k_chol_panel(double *A, int64_t lda, int n, int k0, const int *__restrict__ info)
{
    __shared__ double d[NB * NB]; // L11, column-major (its upper triangle is not read)
    if (*info) return;
    const int i = k0 + NB + blockIdx.x * 64 + threadIdx.x;
    double *R = A + (int64_t)k0 * lda;
    for (int c = 0; c < NB; c++) d[c * NB + threadIdx.x] = (int)threadIdx.x >= c ? R[(int64_t)c * lda + k0 + threadIdx.x] : 0.0;
    __syncthreads();
    const bool live = i < n;
    double b[NB];
#pragma unroll
    for (int c = 0; c < NB; c++) b[c] = live ? R[(int64_t)c * lda + i] : 0.0;
#pragma unroll
    for (int c = 0; c < NB; c++) {
        b[c] = b[c] / d[c * NB + c];
#pragma unroll
        for (int j = c + 1; j < NB; j++) b[j] = fma(-b[c], d[c * NB + j], b[j]);
    }
    if (live) {
#pragma unroll
        for (int c = 0; c < NB; c++) R[(int64_t)c * lda + i] = b[c];
    }
}

// A22 -= L21 L21' on [k1, n)^2, k1 = k0 + 64: tiles bi >= bj of the lower triangle, four waves of 32 x 32; only entries j <= i are touched
__global__ __launch_bounds__(256) void k_chol_trail(double *__restrict__ A, int64_t lda, int n, int k0, const int *__restrict__ info)
{
    if (*info) return;
    int bi, bj;
    tri_tile(blockIdx.x, &bi, &bj);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, wr = wave >> 1, wc = wave & 1;
    if (bi == bj && wr < wc) return; // (the wave's entries all lie above the diagonal)
    const int k1 = k0 + NB, i0 = k1 + bi * NB + wr * 32, j0 = k1 + bj * NB + wc * 32;
    const double *L = A + (int64_t)k0 * lda;
    v4d acc[2][2];
    mma_f64_zero(acc);
    tile_mma(
        acc, 0, NB, lane, [&](int ii, int k) { return i0 + ii < n ? L[(int64_t)k * lda + i0 + ii] : 0.0; },
        [&](int k, int jj) { return j0 + jj < n ? L[(int64_t)k * lda + j0 + jj] : 0.0; });
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int i = i0 + mma_f64_col(a, lane), j = j0 + mma_f64_row(b, r, lane);
                if (i < n && j <= i) A[(int64_t)j * lda + i] -= acc[a][b][r];
            }
}

// every diagonal block inverted in place (workgroup b: [64 b, 64 b + w)^2): L X = I row by row. Row i of the LDS copy is L's until the step that
// replaces it with X's; thread j owns column j, the entries above the diagonal are zeros that the sums run over.
__global__ __launch_bounds__(64) void k_chol_dinv(double *__restrict__ L, int64_t ldl, int n, const int *__restrict__ info)
{
    __shared__ double s[NB * NB];
    if (*info) return;
    const int k0 = blockIdx.x * NB, w = min(NB, n - k0), j = threadIdx.x;
    double *Lb = L + (int64_t)k0 * ldl + k0;
    for (int c = 0; c < NB; c++) s[j * NB + c] = (j < w && c <= j) ? Lb[(int64_t)c * ldl + j] : (j == c ? 1.0 : 0.0);
    __syncthreads();
    for (int i = 0; i < w; i++) {
        double acc = i == j ? 1.0 : 0.0;
        for (int k = 0; k < i; k++) acc = fma(-s[i * NB + k], s[k * NB + j], acc);
        const double x = acc / s[i * NB + i];
        __syncthreads();
        s[i * NB + j] = x;
        __syncthreads();
    }
    for (int c = 0; c < NB; c++)
        if (j < w && c <= j) Lb[(int64_t)c * ldl + j] = s[j * NB + c];
}

// Where a launch of the two kernels below works: the block of columns [c0, c0 + W) and the rows [c0 + W, rend) under its diagonal block. Within the
// super-blocks (blockIdx.z = the super-block, W = 64, rend = the super-block's end) or across them (W = 256, blockIdx.y = the tile of 64 columns, rend = n).
struct chol_col {
    int c0, W, r0, rend, ct;
};
__device__ __forceinline__ chol_col chol_col_of(int n, int cbase, int W, int within)
{
    chol_col g;
    g.c0 = cbase + (int)blockIdx.z * SB;
    g.W = W;
    g.r0 = g.c0 + W;
    g.rend = within ? min(n, (g.c0 / SB + 1) * SB) : n;
    g.ct = (int)blockIdx.y * NB;
    return g;
}

// P = X22 L21 for a block of columns (full width: rows lie under it): workgroup (t, ct) has the 64 rows from r0 + 64 t and the 64 columns from ct, and
// sums over k from r0 to its last row; X22's diagonal blocks are lower triangular (k <= i). Rows from rend on stay out.
__global__ __launch_bounds__(256) void k_chol_trmm(const double *__restrict__ L, int64_t ldl, int n, int cbase, int W, int within, double *__restrict__ P,
                                                   int64_t ldp, const int *__restrict__ info)
{
    if (*info) return;
    const chol_col g = chol_col_of(n, cbase, W, within);
    if (g.r0 + (int)blockIdx.x * NB >= g.rend) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, wr = wave >> 1, wc = wave & 1;
    const int i0 = g.r0 + blockIdx.x * NB + wr * 32, c0 = g.ct + wc * 32, rend = g.rend;
    const double *Lc = L + (int64_t)(g.c0 + c0) * ldl; // the wave's 32 columns of L21
    v4d acc[2][2];
    mma_f64_zero(acc);
    tile_mma(
        acc, g.r0, i0 + 32, lane, [&](int ii, int k) { return (i0 + ii < rend && k <= i0 + ii) ? L[(int64_t)k * ldl + i0 + ii] : 0.0; },
        [&](int k, int cc) { return k < rend ? Lc[(int64_t)cc * ldl + k] : 0.0; });
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int i = i0 + mma_f64_col(a, lane), c = c0 + mma_f64_row(b, r, lane);
                if (i < rend) P[(int64_t)c * ldp + i] = acc[a][b][r];
            }
}

// X21 = -P X11: the rows under the diagonal block of the block of columns, from the panel buffer and the inverted diagonal block (lower triangular: k >= c)
__global__ __launch_bounds__(256) void k_chol_tscale(double *__restrict__ L, int64_t ldl, int n, int cbase, int W, int within, const double *__restrict__ P,
                                                     int64_t ldp, const int *__restrict__ info)
{
    if (*info) return;
    const chol_col g = chol_col_of(n, cbase, W, within);
    if (g.r0 + (int)blockIdx.x * NB >= g.rend) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, wr = wave >> 1, wc = wave & 1;
    const int i0 = g.r0 + blockIdx.x * NB + wr * 32, c0 = g.ct + wc * 32, rend = g.rend;
    const double *Xd = L + (int64_t)g.c0 * ldl + g.c0; // X11
    v4d acc[2][2];
    mma_f64_zero(acc);
    tile_mma(
        acc, c0, g.W, lane, [&](int ii, int k) { return i0 + ii < rend ? P[(int64_t)k * ldp + i0 + ii] : 0.0; },
        [&](int k, int cc) { return k >= c0 + cc ? Xd[(int64_t)(c0 + cc) * ldl + k] : 0.0; });
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int i = i0 + mma_f64_col(a, lane), c = c0 + mma_f64_row(b, r, lane);
                if (i < rend) L[(int64_t)(g.c0 + c) * ldl + i] = -acc[a][b][r];
            }
}

// X = Y' Y for the lower triangular Y = L^-1 in W: the tile (bi, bj), bi >= bj, over k >= its first row; Y[k][i] = 0 for k < i. Both triangles of X.
__global__ __launch_bounds__(256) void k_chol_lauum(const double *__restrict__ W, int64_t ldw, int n, double *__restrict__ X, int64_t ldx,
                                                    const int *__restrict__ info)
{
    if (*info) return;
    int bi, bj;
    tri_tile(blockIdx.x, &bi, &bj);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, wr = wave >> 1, wc = wave & 1;
    if (bi == bj && wr < wc) return; // (the wave's entries all lie above the diagonal)
    const int i0 = bi * NB + wr * 32, j0 = bj * NB + wc * 32;
    v4d acc[2][2];
    mma_f64_zero(acc);
    tile_mma(
        acc, i0, n, lane, [&](int ii, int k) { return (i0 + ii < n && k >= i0 + ii && k < n) ? W[(int64_t)(i0 + ii) * ldw + k] : 0.0; },
        [&](int k, int jj) { return (j0 + jj < n && k >= j0 + jj && k < n) ? W[(int64_t)(j0 + jj) * ldw + k] : 0.0; });
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int i = i0 + mma_f64_col(a, lane), j = j0 + mma_f64_row(b, r, lane);
                if (i < n && j <= i) {
                    const double v = acc[a][b][r];
                    X[(int64_t)j * ldx + i] = v;
                    if (i != j) X[(int64_t)i * ldx + j] = v;
                }
            }
}

int chol_args(const char *who, const void *A, int64_t lda, int n, double lambda, const void *info, bool wants_info)
{
    const std::string w(who);
    if (!A || (wants_info && !info)) return hb_fail(HB_ERR_INVALID, w + ": null argument");
    if (n < 1) return hb_fail(HB_ERR_INVALID, w + ": n < 1");
    if (lda < n) return hb_fail(HB_ERR_INVALID, w + ": leading dimension smaller than n");
    if (!std::isfinite(lambda)) return hb_fail(HB_ERR_INVALID, w + ": lambda must be finite");
    if (hb_device_count() <= 0) return hb_fail(HB_ERR_NO_DEVICE, "no HIP device available: the hibayes GPU engine has no CPU fallback");
    return HB_OK;
}

// the status word of one call, zeroed on the null stream, and its other buffers: "<what> of the n x n matrix" in a refusal's text
int get_info(hb_bufs &m, const hb_cholplan &p, const char *who, int **info)
{
    HB_TRY(m.big(info, (size_t)p.info_bytes / sizeof(int), who, "the status word of the " + hb_dims(p.n) + " matrix"));
    HB_HIP(hipMemsetAsync(*info, 0, p.info_bytes, nullptr));
    return HB_OK;
}
int get_work(hb_bufs &m, size_t bytes, int n, const char *who, const char *what, double **w)
{
    return m.big(w, bytes / sizeof(double), who, std::string(what) + " of the " + hb_dims(n) + " matrix");
}

int factor_launch(const hb_cholplan &p, double *A, int64_t lda, int *info)
{
    for (const hb_cholstep &s : p.steps) {
        hipLaunchKernelGGL(k_chol_diag, dim3(1), dim3(256), 0, nullptr, A, lda, s.k0, s.width, info);
        if (s.row_tiles > 0) {
            hipLaunchKernelGGL(k_chol_panel, dim3((unsigned)s.row_tiles), dim3(64), 0, nullptr, A, lda, p.n, s.k0, info);
            hipLaunchKernelGGL(k_chol_trail, dim3((unsigned)s.tri_tiles), dim3(256), 0, nullptr, A, lda, p.n, s.k0, info);
        }
        HB_HIP(hipGetLastError());
    }
    return HB_OK;
}

int invert_launch(const hb_cholplan &p, double *L, int64_t ldl, double *P, const int *info)
{
    const int n = p.n, per = SB / NB;
    hipLaunchKernelGGL(k_chol_dinv, dim3((unsigned)p.blocks), dim3(64), 0, nullptr, L, ldl, n, info);
    HB_HIP(hipGetLastError());
    // the diagonal super-blocks, all at once: their block columns from the last but one to the first
    for (int lj = per - 2; lj >= 0 && p.blocks > 1; lj--) {
        const dim3 grid((unsigned)(per - 1 - lj), 1, (unsigned)p.super_blocks);
        hipLaunchKernelGGL(k_chol_trmm, grid, dim3(256), 0, nullptr, L, ldl, n, lj * NB, NB, 1, P, p.ldw, info);
        hipLaunchKernelGGL(k_chol_tscale, grid, dim3(256), 0, nullptr, L, ldl, n, lj * NB, NB, 1, P, p.ldw, info);
        HB_HIP(hipGetLastError());
    }
    // the super-block columns from the last but one to the first
    for (int J = p.super_blocks - 2; J >= 0; J--) {
        const dim3 grid((unsigned)((n - (J + 1) * SB + NB - 1) / NB), (unsigned)per, 1);
        hipLaunchKernelGGL(k_chol_trmm, grid, dim3(256), 0, nullptr, L, ldl, n, J * SB, SB, 0, P, p.ldw, info);
        hipLaunchKernelGGL(k_chol_tscale, grid, dim3(256), 0, nullptr, L, ldl, n, J * SB, SB, 0, P, p.ldw, info);
        HB_HIP(hipGetLastError());
    }
    return HB_OK;
}

int fetch_info(const int *info_dev, int32_t *info)
{
    int v = 0;
    HB_HIP(hipMemcpy(&v, info_dev, sizeof v, hipMemcpyDeviceToHost)); // (the null stream: after every launch above)
    if (info) *info = v;
    return HB_OK;
}

} // namespace

extern "C" {

int hb_chol_factor(double *A_dev, int64_t lda, int32_t n, int32_t device, double lambda, int32_t *info)
{
    HB_TRY(chol_args("hb_chol_factor", A_dev, lda, n, lambda, info, true));
    HB_HIP(hipSetDevice(device));
    const hb_cholplan p = hb_cholplan_of(n);
    hb_bufs m;
    int *dinfo = nullptr;
    HB_TRY(get_info(m, p, "hb_chol_factor", &dinfo));
    if (lambda != 0.0) hipLaunchKernelGGL(k_chol_shift, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, A_dev, lda, n, lambda);
    HB_TRY(factor_launch(p, A_dev, lda, dinfo));
    return fetch_info(dinfo, info);
}

int hb_chol_invert_factor(double *L_dev, int64_t lda, int32_t n, int32_t device)
{
    HB_TRY(chol_args("hb_chol_invert_factor", L_dev, lda, n, 0.0, nullptr, false));
    HB_HIP(hipSetDevice(device));
    const hb_cholplan p = hb_cholplan_of(n);
    hb_bufs m;
    int *dinfo = nullptr;
    double *P = nullptr;
    HB_TRY(get_info(m, p, "hb_chol_invert_factor", &dinfo));
    HB_TRY(get_work(m, p.panel_bytes, n, "hb_chol_invert_factor", "a block column", &P));
    HB_TRY(invert_launch(p, L_dev, lda, P, dinfo));
    return fetch_info(dinfo, nullptr);
}

int hb_spd_inverse(double *A_dev, int64_t lda, int32_t n, int32_t device, double lambda, int32_t *info)
{
    HB_TRY(chol_args("hb_spd_inverse", A_dev, lda, n, lambda, info, true));
    HB_HIP(hipSetDevice(device));
    if (n > (1 << 30)) // (8 n^2 bytes would not fit a size_t, and no device holds 2^63 bytes)
        return hb_fail(HB_ERR_HIP, "hb_spd_inverse: out of memory — the work copy of a matrix of more than 2^30 rows cannot be allocated");
    const hb_cholplan p = hb_cholplan_of(n);
    hb_bufs m;
    int *dinfo = nullptr;
    double *P = nullptr, *W = nullptr;
    HB_TRY(get_info(m, p, "hb_spd_inverse", &dinfo));
    HB_TRY(get_work(m, p.panel_bytes, n, "hb_spd_inverse", "a block column", &P));
    HB_TRY(get_work(m, p.work_bytes, n, "hb_spd_inverse", "the work copy", &W));
    hipLaunchKernelGGL(k_chol_copy, dim3((unsigned)n, (unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, A_dev, lda, n, W, p.ldw, lambda, lambda != 0.0 ? 1 : 0);
    HB_HIP(hipGetLastError());
    HB_TRY(factor_launch(p, W, p.ldw, dinfo));
    HB_TRY(invert_launch(p, W, p.ldw, P, dinfo));
    const long long nt = p.blocks;
    hipLaunchKernelGGL(k_chol_lauum, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, nullptr, W, p.ldw, n, A_dev, lda, dinfo);
    HB_HIP(hipGetLastError());
    return fetch_info(dinfo, info);
}

int hb_chol_plan(int32_t n, int32_t cap, int32_t *nb, int64_t *ldw, int64_t *bytes, int32_t *nsteps, int32_t *k0, int32_t *width, int32_t *row_tiles,
                 int64_t *tri_tiles)
{
    if (!nb || !ldw || !bytes || !nsteps || !k0 || !width || !row_tiles || !tri_tiles) return hb_fail(HB_ERR_INVALID, "hb_chol_plan: null argument");
    if (n < 1) return hb_fail(HB_ERR_INVALID, "hb_chol_plan: n < 1");
    const hb_cholplan p = hb_cholplan_of(n);
    if ((size_t)std::max(cap, 0) < p.steps.size()) return hb_fail(HB_ERR_INVALID, "hb_chol_plan: the arrays are shorter than the number of panels");
    *nb = p.nb;
    *ldw = p.ldw;
    bytes[0] = (int64_t)p.factor_bytes;
    bytes[1] = (int64_t)p.invert_bytes;
    bytes[2] = (int64_t)p.inverse_bytes;
    *nsteps = (int32_t)p.steps.size();
    for (size_t s = 0; s < p.steps.size(); s++) {
        k0[s] = p.steps[s].k0;
        width[s] = p.steps[s].width;
        row_tiles[s] = p.steps[s].row_tiles;
        tri_tiles[s] = p.steps[s].tri_tiles;
    }
    return HB_OK;
}

} // extern "C"
