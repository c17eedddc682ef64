// hb_eig.hip — the symmetric eigen-decomposition BSLMM needs (reference src/rm.cpp:46-52, eigen_sym_dc -> LAPACK dsyevd; R/bayes.r:292-294) with
// its two O(n^3) stages on the device. A unit of its own: it shares nothing with the chain kernels' unit but hb_wave.hpp.
//
// Stage 1, dsytrd (uplo = 'L'): Q' A Q = T by Householder reflectors H_k = I - tau_k v_k v_k', v_k[k + 1] = 1, the rest of v_k stored below
// the subdiagonal of column k, beta = -sign(alpha) ||x||, tau = 0 where the part below the subdiagonal is exactly zero. Panel-blocked as dlatrd,
// EIG_NB columns per panel. Both triangles of the trailing square are kept up to date and equal bit for bit (one value is computed per pair
// and stored twice), so p = A22 v is a plain column-major pass. Per column k of a panel (c = k - k0; V, W: the panel's n x EIG_NB buffers):
//     k_eig_colupd   A[k:, k] -= V[k:, :c] W[k, :c]' + W[k:, :c] V[k, :c]'; the workgroups' sums of squares of the part below the subdiagonal
//     k_eig_reflect  one workgroup: those sums in index order, beta, tau, the scale 1 / (alpha - beta); d[k], e[k], tau[k]
//     k_eig_scale    v = x * scale into A and into V[:, c]
//     k_eig_matvec   partial sums of p = A22 v over chunks of columns: a lane owns two rows, 16-byte loads, four columns in flight
//     k_eig_dots     W[:, :c]' v and V[:, :c]' v, a workgroup per dot product
//     k_eig_fold     p = the chunks in order - V (W'v) - W (V'v); W[:, c] = tau p; the workgroups' sums of (tau p)' v
//     k_eig_wfin     W[:, c] -= (tau / 2) (w'v) v
// and after the panel k_eig_trail: A22 -= V W' + W V' on the matrix cores (v_mfma_f64_16x16x4_f64), 64 x 64 tiles of the lower triangle.
// Stage 2, the tridiagonal problem, is the caller's: LAPACK dstemr on the host, or hb_eig_tridiagonal (hb_stedc.hip) on the device.
// Stage 3, dormtr: K = Q Z by block reflectors in compact-WY form, K -= V (T (V' K)) per panel from the last to the first:
//     k_eig_expand   the panel's V with its unit entries and zeros, from A
//     k_eig_gram     V'V, a workgroup per pair of columns;  k_eig_tfac: dlarft's T from it, one workgroup
//     k_eig_vtk      Y = T (V' K): a workgroup per 16 columns of K, its four waves share the rows and are added in wave order
//     k_eig_kupd     K -= V Y, 64 x 64 tiles
// No floating-point atomic anywhere; every sum has one order that depends on n and EIG_NB alone, so two runs agree bit for bit.
#include "hb_internal.hpp"
#include "hb_mma.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>

#ifndef EIG_NB
#define EIG_NB 64 // panel width (32 or 64): 64 halves the traffic of the trailing update and of the back-transformation
#endif

struct hb_eig {
    int n = 0, device = 0;
    int64_t lda = 0;
    double *A = nullptr;       // borrowed: the caller's matrix, overwritten with the reflectors
    bool aligned = false;      // A is 16-byte aligned with an even leading dimension: k_eig_matvec<1>
    int64_t ldv = 0;           // rows of the panel buffers: n rounded up to 64, plus 64 (tiles read past n, never past ldv)
    int64_t ldk = 0;           // leading dimension (and allocated columns) of K: n rounded up to 64
    hipStream_t stream = nullptr;
    double *Vp = nullptr, *Wp = nullptr, *parts = nullptr, *d = nullptr, *e = nullptr, *tau = nullptr, *red = nullptr, *dots = nullptr, *sc = nullptr,
           *S = nullptr, *T = nullptr, *Y = nullptr;
    hb_bufs mem;
};

namespace {

constexpr int NB = EIG_NB;
constexpr int ET = 256;   // threads of the memory-bound kernels
constexpr int TS = 64;    // tile side of the GEMM-shaped kernels
static_assert(NB == 32 || NB == 64, "EIG_NB is 32 or 64");

// chunks of columns of k_eig_matvec on a trailing square of side s: a function of s alone, about 2048 workgroups, chunks of >= 64 columns
inline void mv_plan(int s, int *cpc, int *nchunk)
{
    const int rowblocks = ((s + 1) / 2 + 1 + ET - 1) / ET;
    const int want = std::max(1, 2048 / rowblocks);
    *cpc = std::max(64, (s + want - 1) / want);
    *nchunk = (s + *cpc - 1) / *cpc;
}

// the sum of red[0 .. ET) in a fixed tree; every thread of the workgroup returns it. Not hb_wave.hpp's block_sum: a tree in shared
// memory over the threads, no wave shuffles — another order, and the recorded decompositions the tests compare with were made with it.
__device__ __forceinline__ double block_sum(double v, double *red)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = ET / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

// sum of p[0 .. count): thread t adds p[t], p[t + ET], ... in order, the ET partials in the fixed tree
__device__ __forceinline__ double block_sum_of(const double *__restrict__ p, int count, double *red)
{
    double s = 0.0;
    for (int i = threadIdx.x; i < count; i += ET) s += p[i];
    return block_sum(s, red);
}

// upper triangle <- lower triangle (32 x 32 tiles through LDS): dsytrd with uplo = 'L' reads the lower one only
__global__ __launch_bounds__(ET) void k_eig_mirror(double *__restrict__ A, int64_t lda, int n)
{
    __shared__ double tile[32][33];
    const int tr = blockIdx.x, tc = blockIdx.y; // tile of the lower triangle: tr >= tc
    if (tr < tc) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int cc = ty; cc < 32; cc += 8) {
        const int r = tr * 32 + tx, c = tc * 32 + cc;
        tile[cc][tx] = (r < n && c < n) ? A[(int64_t)c * lda + r] : 0.0;
    }
    __syncthreads();
    for (int cc = ty; cc < 32; cc += 8) {
        const int r = tc * 32 + tx, c = tr * 32 + cc; // entry (r, c) of the upper triangle = entry (c, r) of the lower
        if (r < n && c < n && r < c) A[(int64_t)c * lda + r] = tile[tx][cc];
    }
}

// column k brought up to date from the panel's first c columns (dlatrd, lower: the two dgemv before dlarfg)
__global__ __launch_bounds__(ET) void k_eig_colupd(double *__restrict__ A, int64_t lda, int n, int k, int c, const double *__restrict__ Vp,
                                                   const double *__restrict__ Wp, int64_t ldv, double *__restrict__ sq)
{
    __shared__ double wk[NB], vk[NB], red[ET];
    if ((int)threadIdx.x < c) {
        wk[threadIdx.x] = Wp[(int64_t)threadIdx.x * ldv + k];
        vk[threadIdx.x] = Vp[(int64_t)threadIdx.x * ldv + k];
    }
    __syncthreads();
    const int i = k + blockIdx.x * ET + threadIdx.x;
    double x = 0.0;
    if (i < n) {
        x = A[(int64_t)k * lda + i];
        for (int q = 0; q < c; q++) {
            x = fma(-Vp[(int64_t)q * ldv + i], wk[q], x);
            x = fma(-Wp[(int64_t)q * ldv + i], vk[q], x);
        }
        A[(int64_t)k * lda + i] = x;
    }
    const double s = block_sum((i >= k + 2 && i < n) ? x * x : 0.0, red);
    if (threadIdx.x == 0) sq[blockIdx.x] = s;
}

// dlarfg's scalars, one workgroup. sc[0] = tau, sc[1] = 1 / (alpha - beta) (0 with tau = 0). The rows k0 .. k of the panel's column c are zeroed,
// V[k + 1, c] = 1. Column n - 1 has no reflector: d alone.
__global__ __launch_bounds__(ET) void k_eig_reflect(double *__restrict__ A, int64_t lda, int n, int k, int k0, const double *__restrict__ sq, int nsq,
                                                    double *__restrict__ d, double *__restrict__ e, double *__restrict__ tau, double *__restrict__ sc,
                                                    double *__restrict__ Vc, double *__restrict__ Wc)
{
    __shared__ double red[ET];
    const double xn2 = block_sum_of(sq, nsq, red);
    if ((int)threadIdx.x <= k - k0) {
        Vc[k0 + threadIdx.x] = 0.0;
        Wc[k0 + threadIdx.x] = 0.0;
    }
    if (threadIdx.x != 0) return;
    d[k] = A[(int64_t)k * lda + k];
    if (k + 1 >= n) return;
    const double alpha = A[(int64_t)k * lda + k + 1];
    double beta = alpha, t = 0.0, scale = 0.0;
    if (xn2 != 0.0) {
        beta = -copysign(sqrt(alpha * alpha + xn2), alpha);
        t = (beta - alpha) / beta;
        scale = 1.0 / (alpha - beta);
    }
    e[k] = beta;
    tau[k] = t;
    sc[0] = t;
    sc[1] = scale;
    A[(int64_t)k * lda + k + 1] = beta;
    Vc[k + 1] = 1.0;
}

// v = x / (alpha - beta) below row k + 1: into A (dsytrd's storage of the reflector) and into the panel's column
__global__ __launch_bounds__(ET) void k_eig_scale(double *__restrict__ A, int64_t lda, int n, int k, const double *__restrict__ sc, double *__restrict__ Vc)
{
    const int i = k + 2 + blockIdx.x * ET + threadIdx.x;
    if (i >= n) return;
    const double v = A[(int64_t)k * lda + i] * sc[1];
    A[(int64_t)k * lda + i] = v;
    Vc[i] = v;
}

// parts[chunk][row] = sum over the chunk's columns j, in order, of A[row][j] v[j], on the square [k + 1, n)^2. ALIGNED: a lane owns rows 2 rp,
// 2 rp + 1 (row 2 rp may be k, row 2 rp + 1 may be n: both inside the matrix's allocation, their sums are never read); else one row, 8-byte loads
template <int ALIGNED> __global__ __launch_bounds__(ET) void k_eig_matvec(const double *__restrict__ A, int64_t lda, int n, int k, const double *__restrict__ v,
                                                                            int cpc, double *__restrict__ parts, int64_t ldp)
{
    const int c0 = k + 1 + blockIdx.y * cpc, c1 = min(n, c0 + cpc);
    if (ALIGNED) {
        const int rp = ((k + 1) >> 1) + blockIdx.x * ET + threadIdx.x;
        if (2 * rp >= n) return;
        const d2 *p = reinterpret_cast<const d2 *>(A + (int64_t)c0 * lda) + rp;
        const int64_t st = lda >> 1;
        d2 acc = {0.0, 0.0};
        int j = c0;
        for (; j + 3 < c1; j += 4, p += 4 * st) {
            const d2 a0 = p[0], a1 = p[st], a2 = p[2 * st], a3 = p[3 * st];
            const double v0 = v[j], v1 = v[j + 1], v2 = v[j + 2], v3 = v[j + 3];
            acc.x = fma(a0.x, v0, acc.x); acc.y = fma(a0.y, v0, acc.y);
            acc.x = fma(a1.x, v1, acc.x); acc.y = fma(a1.y, v1, acc.y);
            acc.x = fma(a2.x, v2, acc.x); acc.y = fma(a2.y, v2, acc.y);
            acc.x = fma(a3.x, v3, acc.x); acc.y = fma(a3.y, v3, acc.y);
        }
        for (; j < c1; j++, p += st) {
            const d2 a = p[0];
            const double vj = v[j];
            acc.x = fma(a.x, vj, acc.x); acc.y = fma(a.y, vj, acc.y);
        }
        *(reinterpret_cast<d2 *>(parts + (int64_t)blockIdx.y * ldp) + rp) = acc;
    } else {
        const int i = k + 1 + blockIdx.x * ET + threadIdx.x;
        if (i >= n) return;
        const double *p = A + (int64_t)c0 * lda + i;
        double acc = 0.0;
        int j = c0;
        for (; j + 3 < c1; j += 4, p += 4 * lda) {
            const double a0 = p[0], a1 = p[lda], a2 = p[2 * lda], a3 = p[3 * lda];
            acc = fma(a0, v[j], acc);
            acc = fma(a1, v[j + 1], acc);
            acc = fma(a2, v[j + 2], acc);
            acc = fma(a3, v[j + 3], acc);
        }
        for (; j < c1; j++, p += lda) acc = fma(p[0], v[j], acc);
        parts[(int64_t)blockIdx.y * ldp + i] = acc;
    }
}

// out[b] = W[:, b]' v (b < c), out[c + b] = V[:, b]' v, over the rows k + 1 .. n - 1: a workgroup per dot product
__global__ __launch_bounds__(ET) void k_eig_dots(const double *__restrict__ Vp, const double *__restrict__ Wp, int64_t ldv, int n, int k, int c,
                                                 double *__restrict__ out)
{
    __shared__ double red[ET];
    const int b = blockIdx.x;
    const double *col = (b < c ? Wp + (int64_t)b * ldv : Vp + (int64_t)(b - c) * ldv), *v = Vp + (int64_t)c * ldv;
    double s0 = 0.0, s1 = 0.0;
    int i = k + 1 + threadIdx.x;
    for (; i + ET < n; i += 2 * ET) {
        s0 = fma(col[i], v[i], s0);
        s1 = fma(col[i + ET], v[i + ET], s1);
    }
    if (i < n) s0 = fma(col[i], v[i], s0);
    const double s = block_sum(s0 + s1, red);
    if (threadIdx.x == 0) out[b] = s;
}

// p = the chunks' partials in chunk order, minus V (W'v) + W (V'v); W[:, c] = tau p; the workgroup's sum of (tau p_i) v_i
__global__ __launch_bounds__(ET) void k_eig_fold(const double *__restrict__ parts, int nchunk, int64_t ldp, int n, int k, int c, const double *__restrict__ Vp,
                                                 double *__restrict__ Wp, int64_t ldv, const double *__restrict__ dots, const double *__restrict__ sc,
                                                 double *__restrict__ wv)
{
    __shared__ double dw[NB], dv[NB], red[ET];
    if ((int)threadIdx.x < c) {
        dw[threadIdx.x] = dots[threadIdx.x];
        dv[threadIdx.x] = dots[c + threadIdx.x];
    }
    __syncthreads();
    const int i = k + 1 + blockIdx.x * ET + threadIdx.x;
    double t = 0.0;
    if (i < n) {
        double p = 0.0;
        for (int h = 0; h < nchunk; h++) p += parts[(int64_t)h * ldp + i];
        for (int q = 0; q < c; q++) {
            p = fma(-Vp[(int64_t)q * ldv + i], dw[q], p);
            p = fma(-Wp[(int64_t)q * ldv + i], dv[q], p);
        }
        const double w = sc[0] * p;
        Wp[(int64_t)c * ldv + i] = w;
        t = w * Vp[(int64_t)c * ldv + i];
    }
    const double s = block_sum(t, red);
    if (threadIdx.x == 0) wv[blockIdx.x] = s;
}

// w -= (tau / 2) (w'v) v; every workgroup adds the nwv partial sums in the same order
__global__ __launch_bounds__(ET) void k_eig_wfin(int n, int k, const double *__restrict__ Vc, double *__restrict__ Wc, const double *__restrict__ wv, int nwv,
                                                 const double *__restrict__ sc)
{
    __shared__ double red[ET];
    const double a = -0.5 * sc[0] * block_sum_of(wv, nwv, red);
    const int i = k + 1 + blockIdx.x * ET + threadIdx.x;
    if (i < n) Wc[i] = fma(a, Vc[i], Wc[i]);
}

// The three matrix-core kernels below (hb_mma.hpp: mfma_f64 and its layout): the columns of D run along the index that is contiguous in memory.

// A22 -= V W' + W V' on [k1, n)^2: 64 x 64 tiles bi >= bj of the lower triangle, four waves of 32 x 32; entry (i, j), i >= j, is computed once
// and stored at (i, j) and (j, i). The panel buffers are read past row n (zeros, inside ldv); the matrix is not.
__global__ __launch_bounds__(256) void k_eig_trail(double *__restrict__ A, int64_t lda, int n, int k1, const double *__restrict__ Vp, const double *__restrict__ Wp,
                                                   int64_t ldv)
{
    int bi, bj;
    tri_tile(blockIdx.x, &bi, &bj);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, wr = wave >> 1, wc = wave & 1, lr = lane & 15, q = lane >> 4;
    if (bi == bj && wr < wc) return; // (the wave's entries all lie above the diagonal)
    const int i0 = k1 + bi * TS + wr * 32, j0 = k1 + bj * TS + wc * 32;
    v4d acc[2][2];
    mma_f64_zero(acc);
#pragma unroll 4
    for (int s = 0; s < NB / 4; s++) {
        const int64_t co = (int64_t)(4 * s + q) * ldv;
        double vi[2], wi[2], vj[2], wj[2];
#pragma unroll
        for (int a = 0; a < 2; a++) {
            vi[a] = Vp[co + i0 + 16 * a + lr];
            wi[a] = Wp[co + i0 + 16 * a + lr];
            vj[a] = Vp[co + j0 + 16 * a + lr];
            wj[a] = Wp[co + j0 + 16 * a + lr];
        }
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++) {
                acc[a][b] = mfma_f64(wj[b], vi[a], acc[a][b]); // D[j][i] += W[j][c] V[i][c]
                acc[a][b] = mfma_f64(vj[b], wi[a], acc[a][b]); //          + V[j][c] W[i][c]
            }
    }
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int i = i0 + mma_f64_col(a, lane), j = j0 + mma_f64_row(b, r, lane);
                if (i < n && j <= i) {
                    const double nv = A[(int64_t)j * lda + i] - acc[a][b][r];
                    A[(int64_t)j * lda + i] = nv;
                    if (i != j) A[(int64_t)i * lda + j] = nv;
                }
            }
}

// the panel's reflectors, explicit: V[i, c] = 0 (i <= k), 1 (i = k + 1), A[i, k] (k + 1 < i < n), 0 (i >= n or c >= nbp), k = k0 + c; rows rbase .. ldv - 1
__global__ __launch_bounds__(ET) void k_eig_expand(const double *__restrict__ A, int64_t lda, int n, int k0, int nbp, int rbase, double *__restrict__ Vp, int64_t ldv)
{
    const int64_t i = (int64_t)rbase + (int64_t)blockIdx.x * ET + threadIdx.x;
    const int c = blockIdx.y, k = k0 + c;
    if (i >= ldv) return;
    double v = 0.0;
    if (c < nbp && i < n) {
        if (i == k + 1) v = 1.0;
        else if (i > k + 1) v = A[(int64_t)k * lda + i];
    }
    Vp[(int64_t)c * ldv + i] = v;
}

// S[a][b] = V[:, a]' V[:, b] for a < b, rows b + k0 + 1 .. n - 1 (V[:, b] is zero above): a workgroup per pair, blockIdx = b (b - 1) / 2 + a
__global__ __launch_bounds__(ET) void k_eig_gram(const double *__restrict__ Vp, int64_t ldv, int n, int k0, double *__restrict__ S)
{
    __shared__ double red[ET];
    int a, b;
    tri_tile(blockIdx.x, &b, &a); // (the strict triangle: b - 1 >= a)
    b++;
    const double *x = Vp + (int64_t)a * ldv, *y = Vp + (int64_t)b * ldv;
    double s0 = 0.0, s1 = 0.0;
    int i = k0 + b + 1 + threadIdx.x;
    for (; i + ET < n; i += 2 * ET) {
        s0 = fma(x[i], y[i], s0);
        s1 = fma(x[i + ET], y[i + ET], s1);
    }
    if (i < n) s0 = fma(x[i], y[i], s0);
    const double s = block_sum(s0 + s1, red);
    if (threadIdx.x == 0) S[a * NB + b] = s;
}

// dlarft (forward, columnwise): T[c][c] = tau_c, T[0:c, c] = -tau_c T[0:c, 0:c] (V[:, 0:c]' v_c); one workgroup of NB threads, thread r owns row r.
// T is stored row-major, NB x NB, zero below the diagonal and in the columns past nbp.
__global__ __launch_bounds__(NB) void k_eig_tfac(const double *__restrict__ S, const double *__restrict__ tau, int k0, int nbp, double *__restrict__ T)
{
    __shared__ double t[NB][NB + 1], z[NB];
    const int r = threadIdx.x;
    for (int c = 0; c < NB; c++) t[r][c] = 0.0;
    __syncthreads();
    for (int c = 0; c < nbp; c++) {
        const double tc = tau[k0 + c];
        z[r] = r < c ? -tc * S[r * NB + c] : 0.0;
        __syncthreads();
        double s = 0.0;
        for (int q = r; q < c; q++) s = fma(t[r][q], z[q], s);
        if (r < c) t[r][c] = s;
        if (r == c) t[r][c] = tc;
        __syncthreads();
    }
    for (int c = 0; c < NB; c++) T[r * NB + c] = t[r][c];
}

// Y[:, j] = T (V' K[:, j]) for the 16 columns j of the workgroup. Wave w takes the rows rbase + 16 (w + 4 t) .. + 15, t = 0, 1, ...; a lane loads four
// consecutive rows of one column of K and of V (two 16-byte loads each) and feeds them to four MFMAs, k-slot q of step s = row 4 q + s. The waves'
// sums are added in wave order, then T (upper triangular) is applied in plain fp64. K and V are read up to row ldk - 1 (zeros past n).
__global__ __launch_bounds__(256) void k_eig_vtk(const double *__restrict__ K, int64_t ldk, int n, int rbase, const double *__restrict__ Vp, int64_t ldv,
                                                 const double *__restrict__ T, double *__restrict__ Y)
{
    __shared__ double part[4][NB][17], y0[NB][17];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, q = lane >> 4;
    const int j0 = blockIdx.x * 16;
    v4d acc[NB / 16];
#pragma unroll
    for (int t = 0; t < NB / 16; t++) acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};
    const double *kc = K + (int64_t)(j0 + lr) * ldk;
    for (int i0 = rbase + 16 * wave; i0 < n; i0 += 64) {
        const d2 k01 = *reinterpret_cast<const d2 *>(kc + i0 + 4 * q), k23 = *reinterpret_cast<const d2 *>(kc + i0 + 4 * q + 2);
#pragma unroll
        for (int t = 0; t < NB / 16; t++) {
            const double *vc = Vp + (int64_t)(16 * t + lr) * ldv + i0 + 4 * q;
            const d2 v01 = *reinterpret_cast<const d2 *>(vc), v23 = *reinterpret_cast<const d2 *>(vc + 2);
            acc[t] = mfma_f64(v01.x, k01.x, acc[t]); // D[c][j] += V[i][c] K[i][j]
            acc[t] = mfma_f64(v01.y, k01.y, acc[t]);
            acc[t] = mfma_f64(v23.x, k23.x, acc[t]);
            acc[t] = mfma_f64(v23.y, k23.y, acc[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < NB / 16; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) part[wave][16 * t + q + 4 * r][lr] = acc[t][r];
    __syncthreads();
    for (int x = threadIdx.x; x < NB * 16; x += 256) {
        const int c = x >> 4, jj = x & 15;
        y0[c][jj] = ((part[0][c][jj] + part[1][c][jj]) + part[2][c][jj]) + part[3][c][jj];
    }
    __syncthreads();
    for (int x = threadIdx.x; x < NB * 16; x += 256) {
        const int c = x >> 4, jj = x & 15;
        double s = 0.0;
        for (int p = c; p < NB; p++) s = fma(T[c * NB + p], y0[p][jj], s);
        Y[(int64_t)(j0 + jj) * NB + c] = s;
    }
}

// K -= V Y on the rows rbase .. ldk - 1, all ldk columns: 64 x 64 tiles, four waves of 32 x 32. No guards: K is padded to whole tiles, V is zero
// above the panel's first reflector and past n, so those rows keep their values.
__global__ __launch_bounds__(256) void k_eig_kupd(double *__restrict__ K, int64_t ldk, int rbase, const double *__restrict__ Vp, int64_t ldv, const double *__restrict__ Y)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, wr = wave >> 1, wc = wave & 1, lr = lane & 15, q = lane >> 4;
    const int i0 = rbase + blockIdx.x * TS + wr * 32, j0 = blockIdx.y * TS + wc * 32;
    v4d acc[2][2];
    mma_f64_zero(acc);
#pragma unroll 4
    for (int s = 0; s < NB / 4; s++) {
        double vi[2], yj[2];
#pragma unroll
        for (int a = 0; a < 2; a++) {
            vi[a] = Vp[(int64_t)(4 * s + q) * ldv + i0 + 16 * a + lr];
            yj[a] = Y[(int64_t)(j0 + 16 * a + lr) * NB + 4 * s + q];
        }
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++) acc[a][b] = mfma_f64(yj[b], vi[a], acc[a][b]); // D[j][i] += Y[c][j] V[i][c]
    }
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                double *p = K + (int64_t)(j0 + mma_f64_row(b, r, lane)) * ldk + i0 + mma_f64_col(a, lane);
                *p -= acc[a][b][r];
            }
}

__global__ __launch_bounds__(ET) void k_eig_identity(double *__restrict__ K, int64_t ldk, int n)
{
    const int i = blockIdx.x * ET + threadIdx.x;
    if (i < n) K[(int64_t)i * ldk + i] = 1.0;
}

inline unsigned blocks(int64_t count) { return (unsigned)std::max<int64_t>(1, (count + ET - 1) / ET); }

int no_device(const char *who)
{
    if (hb_device_count() <= 0) return hb_fail(HB_ERR_NO_DEVICE, "no HIP device available: the hibayes GPU engine has no CPU fallback");
    (void)who;
    return HB_OK;
}

// one column of a panel: everything of dlatrd's loop body
int reduce_column(hb_eig *h, int k, int k0)
{
    const int n = h->n, c = k - k0;
    double *Vc = h->Vp + (int64_t)c * h->ldv, *Wc = h->Wp + (int64_t)c * h->ldv;
    double *sq = h->red, *wv = h->red + blocks(n);
    const unsigned nsq = blocks(n - k);
    hipLaunchKernelGGL(k_eig_colupd, dim3(nsq), dim3(ET), 0, h->stream, h->A, h->lda, n, k, c, h->Vp, h->Wp, h->ldv, sq);
    hipLaunchKernelGGL(k_eig_reflect, dim3(1), dim3(ET), 0, h->stream, h->A, h->lda, n, k, k0, sq, (int)nsq, h->d, h->e, h->tau, h->sc, Vc, Wc);
    HB_HIP(hipGetLastError());
    if (k + 1 >= n) return HB_OK;
    const int s = n - k - 1;
    if (s > 1) hipLaunchKernelGGL(k_eig_scale, dim3(blocks(s - 1)), dim3(ET), 0, h->stream, h->A, h->lda, n, k, h->sc, Vc);
    int cpc, nchunk;
    mv_plan(s, &cpc, &nchunk);
    if (h->aligned) {
        const int npairs = ((n - 1) >> 1) - ((k + 1) >> 1) + 1;
        hipLaunchKernelGGL(k_eig_matvec<1>, dim3(blocks(npairs), (unsigned)nchunk), dim3(ET), 0, h->stream, h->A, h->lda, n, k, Vc, cpc, h->parts, h->ldv);
    } else
        hipLaunchKernelGGL(k_eig_matvec<0>, dim3(blocks(s), (unsigned)nchunk), dim3(ET), 0, h->stream, h->A, h->lda, n, k, Vc, cpc, h->parts, h->ldv);
    if (c > 0) hipLaunchKernelGGL(k_eig_dots, dim3((unsigned)(2 * c)), dim3(ET), 0, h->stream, h->Vp, h->Wp, h->ldv, n, k, c, h->dots);
    const unsigned nwv = blocks(s);
    hipLaunchKernelGGL(k_eig_fold, dim3(nwv), dim3(ET), 0, h->stream, h->parts, nchunk, h->ldv, n, k, c, h->Vp, h->Wp, h->ldv, h->dots, h->sc, wv);
    hipLaunchKernelGGL(k_eig_wfin, dim3(nwv), dim3(ET), 0, h->stream, n, k, Vc, Wc, wv, (int)nwv, h->sc);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int reduce_all(hb_eig *h)
{
    const int n = h->n;
    const unsigned nt32 = (unsigned)((n + 31) / 32);
    hipLaunchKernelGGL(k_eig_mirror, dim3(nt32, nt32), dim3(ET), 0, h->stream, h->A, h->lda, n);
    HB_HIP(hipGetLastError());
    for (int k0 = 0; k0 < n; k0 += NB) {
        const int k1 = std::min(n, k0 + NB);
        for (int k = k0; k < k1; k++) HB_TRY(reduce_column(h, k, k0));
        if (k1 < n) {
            const long long nt = (n - k1 + TS - 1) / TS;
            hipLaunchKernelGGL(k_eig_trail, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, h->stream, h->A, h->lda, n, k1, h->Vp, h->Wp, h->ldv);
            HB_HIP(hipGetLastError());
        }
    }
    return HB_OK;
}

// K <- Q K by the panels' block reflectors from the last to the first (dormtr); K is ldk x ldk, zero past n
int back_transform(hb_eig *h, double *K)
{
    const int n = h->n;
    const int nref = n - 1; // reflectors k = 0 .. n - 2
    for (int k0 = (nref - 1) / NB * NB; nref > 0 && k0 >= 0; k0 -= NB) {
        const int nbp = std::min(NB, nref - k0);
        const int rbase = (k0 + 1) / TS * TS;
        hipLaunchKernelGGL(k_eig_expand, dim3(blocks(h->ldv - rbase), (unsigned)NB), dim3(ET), 0, h->stream, h->A, h->lda, n, k0, nbp, rbase, h->Vp, h->ldv);
        if (nbp > 1) hipLaunchKernelGGL(k_eig_gram, dim3((unsigned)(nbp * (nbp - 1) / 2)), dim3(ET), 0, h->stream, h->Vp, h->ldv, n, k0, h->S);
        hipLaunchKernelGGL(k_eig_tfac, dim3(1), dim3(NB), 0, h->stream, h->S, h->tau, k0, nbp, h->T);
        hipLaunchKernelGGL(k_eig_vtk, dim3((unsigned)(h->ldk / 16)), dim3(256), 0, h->stream, K, h->ldk, n, rbase, h->Vp, h->ldv, h->T, h->Y);
        hipLaunchKernelGGL(k_eig_kupd, dim3((unsigned)((h->ldk - rbase) / TS), (unsigned)(h->ldk / TS)), dim3(256), 0, h->stream, K, h->ldk, rbase, h->Vp,
                           h->ldv, h->Y);
        HB_HIP(hipGetLastError());
    }
    return HB_OK;
}

} // namespace

extern "C" {

// the caller's host matrix on the device, with an even leading dimension (hb_eig_reduce's fast mat-vec); released with hb_eig_release
int hb_eig_upload(const double *A_host, int64_t lda_host, int32_t n, int32_t device, double **A_dev, int64_t *lda)
{
    if (A_dev) *A_dev = nullptr;
    if (!A_host || !A_dev || !lda) return hb_fail(HB_ERR_INVALID, "hb_eig_upload: null argument");
    if (n < 1 || lda_host < n) return hb_fail(HB_ERR_INVALID, "hb_eig_upload: n < 1 or a leading dimension smaller than n");
    HB_TRY(no_device("hb_eig_upload"));
    HB_HIP(hipSetDevice(device));
    const int64_t ld = (int64_t)n + (n & 1);
    hb_bufs mem;
    double *p = nullptr;
    HB_TRY(mem.big(&p, (size_t)ld * (size_t)n, "hb_eig_upload", "the " + hb_dims(n) + " matrix"));
    hipError_t e = ld != n ? hipMemset(p, 0, sizeof(double) * (size_t)ld * (size_t)n) : hipSuccess;
    if (e == hipSuccess)
        e = hipMemcpy2D(p, sizeof(double) * (size_t)ld, A_host, sizeof(double) * (size_t)lda_host, sizeof(double) * (size_t)n, (size_t)n, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hb_fail(HB_ERR_HIP, std::string("hb_eig_upload: ") + hipGetErrorString(e));
    mem.release(p); // the caller's from here (hb_eig_release)
    *A_dev = p;
    *lda = ld;
    return HB_OK;
}

// LAPACK dsytrd, uplo = 'L' (the first stage of the dsyevd behind eigen_sym_dc, reference src/rm.cpp:46-52)
int hb_eig_reduce(double *A_dev, int64_t lda, int32_t n, int32_t device, double *d_host, double *e_host, hb_eig **out)
{
    if (out) *out = nullptr;
    if (!A_dev || !d_host || !out || (n > 1 && !e_host)) return hb_fail(HB_ERR_INVALID, "hb_eig_reduce: null argument");
    if (n < 1) return hb_fail(HB_ERR_INVALID, "hb_eig_reduce: n < 1");
    if (lda < n) return hb_fail(HB_ERR_INVALID, "hb_eig_reduce: leading dimension smaller than n");
    HB_TRY(no_device("hb_eig_reduce"));
    HB_HIP(hipSetDevice(device));
    hb_eig *h = new hb_eig();
    h->n = n;
    h->device = device;
    h->A = A_dev;
    h->lda = lda;
    h->aligned = !(lda & 1) && !(reinterpret_cast<uintptr_t>(A_dev) & 15u);
    h->ldk = ((int64_t)n + TS - 1) / TS * TS;
    h->ldv = h->ldk + TS;
    int maxchunk = 1;
    for (int s = 1; s < n; s++) {
        int cpc, nchunk;
        mv_plan(s, &cpc, &nchunk);
        maxchunk = std::max(maxchunk, nchunk);
    }
    auto build = [&]() -> int {
        HB_HIP(hipStreamCreate(&h->stream));
        HB_TRY(h->mem.zeroed(&h->Vp, (size_t)h->ldv * NB, h->stream));
        HB_TRY(h->mem.zeroed(&h->Wp, (size_t)h->ldv * NB, h->stream));
        HB_TRY(h->mem.zeroed(&h->parts, (size_t)h->ldv * (size_t)maxchunk, h->stream));
        HB_TRY(h->mem.zeroed(&h->d, (size_t)n, h->stream));
        HB_TRY(h->mem.zeroed(&h->e, (size_t)n, h->stream));
        HB_TRY(h->mem.zeroed(&h->tau, (size_t)n + NB, h->stream));
        HB_TRY(h->mem.zeroed(&h->red, (size_t)2 * blocks(n), h->stream));
        HB_TRY(h->mem.zeroed(&h->dots, (size_t)2 * NB, h->stream));
        HB_TRY(h->mem.zeroed(&h->sc, 4, h->stream));
        HB_TRY(h->mem.zeroed(&h->S, (size_t)NB * NB, h->stream));
        HB_TRY(h->mem.zeroed(&h->T, (size_t)NB * NB, h->stream));
        HB_TRY(h->mem.zeroed(&h->Y, (size_t)NB * (size_t)h->ldk, h->stream));
        HB_TRY(reduce_all(h));
        HB_HIP(hipMemcpyAsync(d_host, h->d, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
        if (n > 1) HB_HIP(hipMemcpyAsync(e_host, h->e, sizeof(double) * (size_t)(n - 1), hipMemcpyDeviceToHost, h->stream));
        HB_HIP(hipStreamSynchronize(h->stream));
        for (int i = 0; i < n; i++)
            if (!std::isfinite(d_host[i]) || (i < n - 1 && !std::isfinite(e_host[i])))
                return hb_fail(HB_ERR_INVALID, "hb_eig_reduce: the matrix holds a non-finite value (its tridiagonal form is not finite)");
        return HB_OK;
    };
    const int rc = build();
    if (rc) {
        hb_eig_destroy(h);
        return rc;
    }
    *out = h;
    return HB_OK;
}

// tau of the n - 1 reflectors (dsytrd's TAU), for the tests
int hb_eig_tau(hb_eig *h, double *tau_host)
{
    if (!h || !tau_host) return hb_fail(HB_ERR_INVALID, "hb_eig_tau: null handle or argument");
    HB_HIP(hipSetDevice(h->device));
    if (h->n > 1) HB_HIP(hipMemcpy(tau_host, h->tau, sizeof(double) * (size_t)(h->n - 1), hipMemcpyDeviceToHost));
    return HB_OK;
}

// LAPACK dormtr (side = 'L', uplo = 'L', trans = 'N'): K = Q Z, the last stage of dsyevd (reference src/rm.cpp:46-52; what R/bayes.r:292-294
// hands to Bayes() as Ki). Z_host = NULL: Z = I, K = Q (dorgtr).
int hb_eig_vectors(hb_eig *h, const double *Z_host, int64_t ldz, double **K_dev, int64_t *ldk)
{
    if (K_dev) *K_dev = nullptr;
    if (!h) return hb_fail(HB_ERR_INVALID, "hb_eig_vectors: null handle");
    if (!K_dev || !ldk) return hb_fail(HB_ERR_INVALID, "hb_eig_vectors: null argument");
    const int n = h->n;
    if (Z_host && ldz < n) return hb_fail(HB_ERR_INVALID, "hb_eig_vectors: leading dimension smaller than n");
    HB_TRY(no_device("hb_eig_vectors"));
    HB_HIP(hipSetDevice(h->device));
    hb_bufs mem;
    double *K = nullptr;
    HB_TRY(mem.big(&K, (size_t)h->ldk * (size_t)h->ldk, "hb_eig_vectors", "the " + hb_dims(n) + " eigenvector matrix"));
    HB_HIP(hipMemsetAsync(K, 0, sizeof(double) * (size_t)h->ldk * (size_t)h->ldk, h->stream));
    if (Z_host) {
        // column strips of at most 256 MB: the pageable copy is staged strip by strip
        const int strip = (int)std::max<int64_t>(1, ((int64_t)256 << 20) / ((int64_t)sizeof(double) * n));
        for (int j = 0; j < n; j += strip)
            HB_HIP(hipMemcpy2DAsync(K + (int64_t)j * h->ldk, sizeof(double) * (size_t)h->ldk, Z_host + (int64_t)j * ldz, sizeof(double) * (size_t)ldz,
                                    sizeof(double) * (size_t)n, (size_t)std::min(strip, n - j), hipMemcpyHostToDevice, h->stream));
    } else
        hipLaunchKernelGGL(k_eig_identity, dim3(blocks(n)), dim3(ET), 0, h->stream, K, h->ldk, n);
    HB_HIP(hipGetLastError());
    HB_TRY(back_transform(h, K));
    HB_HIP(hipStreamSynchronize(h->stream));
    mem.release(K); // the caller's from here (hb_eig_release)
    *K_dev = K;
    *ldk = h->ldk;
    return HB_OK;
}

// hb_eig_vectors for a Z that is on the device already (hb_eig_tridiagonal): K = Q Z in place in Z's buffer, whose ownership passes to *K_dev
// (hb_eig_release frees it; on failure the buffer stays the caller's). ldz must be the handle's ldk: n rounded up to 64, that many columns, padding zero.
int hb_eig_vectors_dev(hb_eig *h, double *Z_dev, int64_t ldz, double **K_dev, int64_t *ldk)
{
    if (K_dev) *K_dev = nullptr;
    if (!h) return hb_fail(HB_ERR_INVALID, "hb_eig_vectors_dev: null handle");
    if (!Z_dev || !K_dev || !ldk) return hb_fail(HB_ERR_INVALID, "hb_eig_vectors_dev: null argument");
    if (ldz != h->ldk) return hb_fail(HB_ERR_INVALID, "hb_eig_vectors_dev: the leading dimension of Z must be n rounded up to 64");
    HB_TRY(no_device("hb_eig_vectors_dev"));
    HB_HIP(hipSetDevice(h->device));
    HB_TRY(back_transform(h, Z_dev));
    HB_HIP(hipStreamSynchronize(h->stream));
    *K_dev = Z_dev;
    *ldk = h->ldk;
    return HB_OK;
}

// an n x n device matrix (K of hb_eig_vectors, or the reduced A with its reflectors) to a host column-major array
int hb_eig_download(const double *M_dev, int64_t ld_dev, int32_t n, int32_t device, double *M_host, int64_t ld_host)
{
    if (!M_dev || !M_host) return hb_fail(HB_ERR_INVALID, "hb_eig_download: null argument");
    if (n < 1 || ld_dev < n || ld_host < n) return hb_fail(HB_ERR_INVALID, "hb_eig_download: n < 1 or a leading dimension smaller than n");
    HB_TRY(no_device("hb_eig_download"));
    HB_HIP(hipSetDevice(device));
    HB_HIP(hipMemcpy2D(M_host, sizeof(double) * (size_t)ld_host, M_dev, sizeof(double) * (size_t)ld_dev, sizeof(double) * (size_t)n, (size_t)n, hipMemcpyDeviceToHost));
    return HB_OK;
}

void hb_eig_release(double *M_dev)
{
    hb_free_released(M_dev);
}

void hb_eig_destroy(hb_eig *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->mem.clear();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

} // extern "C"
