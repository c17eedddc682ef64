// hb_grm.hip — BSLMM's dense side on the device: make_grm() of the reference (src/rm.cpp:5-53) from the resident int8
// genotypes, and the polygenic block of one iteration of Bayes() (src/Bayes.cpp:518-552) on the eigenvectors K of that matrix.
// A unit of its own: it shares nothing with the chain kernels' unit but hb_wave.hpp.
//
// GRM. G = Z Z' with Z = M - 1 c'/n (c: the markers' column sums). With S = M M', a_i = sum_k c_k M_ik and C = sum_k c_k^2 — all exact
// integers — the centred cross-product is
//     raw_ij = S_ij - (a_i + a_j) / n + C / n^2 .
// S runs on the matrix cores (v_mfma_i32_32x32x32_i8) in int32 over chunks of GRM_KCHUNK markers, int64 across chunks; a and C are int64 /
// 128-bit integer sums. One fp64 expression (grm_raw below) turns the integers into raw_ij, whatever the tiling; then G = raw /
// mean(diag raw) and diag += lambda (src/rm.cpp:37, :46). One triangle is computed, both are written.
//
// Polygenic block, K n x n column-major fp64 with an even leading dimension (every column 16-byte aligned):
//     k_poly_dot<0>   t = K'(yadj + k_old): a wave per contiguous column; its epilogue forms eval_j (:531), draws z_j (Philox purpose 5) and
//                     leaves w_j = (eval_j / vare) t_j + sqrt(max(eval_j, 0)) z_j
//     k_poly_kw       partial sums of k_new = K w: a lane owns two rows and walks a chunk of columns with 16-byte loads, parts[chunk][row]
//     k_poly_fold     k_new = the chunks' partials re-added in chunk order; yadj += k_old - k_new, u -= k_old - k_new (:537-540), the
//                     residual's fp32 mirror as k_axpy leaves it
//     k_poly_dot<1>   Kg = K' k_new and the terms Kg_j^2 / Kval_j (:543-544)
//     k_poly_final    q = their sum in index order, vb = (q + s2vara dfvara) / chisq (:546-547), the check of :533
// No floating-point atomic anywhere: every sum has one fixed order and two runs agree bit for bit.
#include "hb_internal.hpp"
#include "hb_rng.hpp"
#include "hb_mma.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

struct hb_poly {
    int n = 0;
    int64_t ld = 0;          // leading dimension of K in doubles, even
    const double *K = nullptr;
    double *K_own = nullptr; // the uploaded copy (nullptr: K is borrowed)
    double *Kval = nullptr, *k_cur = nullptr, *k_sum = nullptr, *t = nullptr, *w = nullptr, *ev = nullptr, *Kg = nullptr, *qt = nullptr, *parts = nullptr,
           *vec = nullptr;   // n-long device vectors (each allocated with ld + 2 doubles); parts: nchunk x ld
    double *st = nullptr;    // device: [0] vb, [1] q, [2] flag of :533 (1: not positive definite)
    double *h_st = nullptr;  // pinned mirror, filled by the sweep's fetch
    int cpc = 0, nchunk = 0; // columns per chunk of k_poly_kw, chunks
    int stored = 0;          // records accumulated in k_sum
    hb_bufs mem;             // every buffer above but a borrowed K
};

namespace {

// ---------------------------------------------------------------------------------------------------------------------------------
// GRM
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int GT = 128;            // individuals per side of a workgroup's tile (4 waves, 64 x 64 each)
constexpr int GK = 64;             // markers per step (a staged row takes hb_mma.hpp's MMA_CS bytes: the same conflict-free operand reads)
constexpr int GRM_KCHUNK = 65536;  // markers summed in int32: 128^2 * 65536 = 2^30 < 2^31 for every int8 code

// THE expression: raw_ij = (S_ij - (a_i + a_j) / n) + C / n^2, with S, a_i + a_j exact integers, cn2 = (double)C / (n * n)
// formed once on the host. |error| <= 4 eps (|S_ij| + |a_i + a_j| / n + C / n^2).
__device__ __forceinline__ double grm_raw(long long s, long long ai, long long aj, double nd, double cn2)
{
    const double t2 = (double)(ai + aj) / nd;
    return ((double)s - t2) + cn2;
}

// bytes rr of four words -> one word (a 4 x 4 byte transpose, one row of it)
__device__ __forceinline__ unsigned tr_row(unsigned d0, unsigned d1, unsigned d2_, unsigned d3, int rr)
{
    const int sh = 8 * rr;
    return ((d0 >> sh) & 0xffu) | (((d1 >> sh) & 0xffu) << 8) | (((d2_ >> sh) & 0xffu) << 16) | (((d3 >> sh) & 0xffu) << 24);
}

// stage rows [row0, row0 + 128) x markers [kk, kk + 64) of the column-major int8 matrix into LDS as [row][marker]: thread -> four rows
// (tid & 31) x four markers of two marker groups; the global loads run along the rows (128 contiguous bytes per marker and half wave)
__device__ __forceinline__ void grm_stage(const int8_t *__restrict__ X, int64_t ld, int n, int row0, int kk, int k1, char *__restrict__ lds, int tid)
{
    const int rg = tid & 31, kg = tid >> 5;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int kq = (kg + 8 * h) * 4;
        unsigned d[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int k = kk + kq + q;
            d[q] = k < k1 ? *reinterpret_cast<const unsigned *>(X + (int64_t)k * ld + row0 + rg * 4) : 0u;
        }
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const int row = rg * 4 + rr;
            const unsigned v = (row0 + row < n) ? tr_row(d[0], d[1], d[2], d[3], rr) : 0u;
            *reinterpret_cast<unsigned *>(lds + row * MMA_CS + kq) = v;
        }
    }
}

// S (+)= M[:, k0:k1] M[:, k0:k1]' on the tiles bi >= bj of the 128 x 128 tiling. The tile's entries (i in tile bi, j in tile bj, j <= i) are
// written at S[i * ldS + j] — the lanes of the C layout run along j, so the stores are contiguous; read as column-major that is the UPPER
// triangle, and k_grm_combine fills both from it.
__global__ __launch_bounds__(256) void k_grm_tile(const int8_t *__restrict__ X, int64_t ld, int n, int k0, int k1, long long *__restrict__ S, int64_t ldS, int first)
{
    __shared__ __attribute__((aligned(16))) char sa[GT * MMA_CS], sb[GT * MMA_CS];
    int bi, bj;
    tri_tile(blockIdx.x, &bi, &bj);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wr = wave >> 1, wc = wave & 1;
    const char *ra = sa + wr * 64 * MMA_CS + mma_i8_operand(lane, MMA_CS);
    const char *rb = sb + wc * 64 * MMA_CS + mma_i8_operand(lane, MMA_CS);
    v16i acc[2][2];
    mma_i8_zero(acc);
    for (int kk = k0; kk < k1; kk += GK) {
        __syncthreads(); // everybody is done reading the previous step
        grm_stage(X, ld, n, bi * GT, kk, k1, sa, tid);
        grm_stage(X, ld, n, bj * GT, kk, k1, sb, tid);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < GK; ks += 32) mma_i8_step(acc, ra + ks, rb + ks, MMA_CS);
    }
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int i = bi * GT + wr * 64 + mma_i8_row(a, r, lane);
                const int j = bj * GT + wc * 64 + mma_i8_col(b, lane);
                if (i < n && j <= i) {
                    long long *p = S + (int64_t)i * ldS + j;
                    *p = first ? (long long)acc[a][b][r] : *p + (long long)acc[a][b][r];
                }
            }
}

// a_i = sum_k c_k M_ik over the markers of slice blockIdx.y: integer atomics, exact and order-independent
__global__ __launch_bounds__(256) void k_grm_a(const int8_t *__restrict__ X, int64_t ld, int n, int m, int kslice, const double *__restrict__ s1,
                                               unsigned long long *__restrict__ a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int k0 = blockIdx.y * kslice, k1 = min(m, k0 + kslice);
    long long s = 0;
    for (int k = k0; k < k1; k++) s += (long long)s1[k] * (long long)X[(int64_t)k * ld + i];
    atomicAdd(a + i, (unsigned long long)s);
}

__global__ __launch_bounds__(256) void k_grm_diag(const long long *__restrict__ S, int64_t ldS, int n, const long long *__restrict__ a, double nd,
                                                  double cn2, double *__restrict__ d)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) d[i] = grm_raw(S[(int64_t)i * ldS + i], a[i], a[i], nd, cn2);
}

// one workgroup: out[0] = mean of d[0 .. n) — thread t adds d[t], d[t + 256], ... in order, the 256 partials are added in a fixed tree
__global__ __launch_bounds__(256) void k_grm_mean(const double *__restrict__ d, int n, double *__restrict__ out)
{
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += d[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0] / (double)n;
}

// in place: the int64 sums of the computed triangle -> the fp64 matrix, both triangles. 32 x 32 tiles tr <= tc; tile[cc][rr] = entry
// (row tr * 32 + rr, column tc * 32 + cc), written there and, transposed through LDS, at the mirrored tile
__global__ __launch_bounds__(256) void k_grm_combine(double *__restrict__ G, int64_t ldG, int n, const long long *__restrict__ a, double nd, double cn2,
                                                     const double *__restrict__ mean, double lambda, int raw)
{
    __shared__ double tile[32][33];
    const int tr = blockIdx.x, tc = blockIdx.y;
    if (tr > tc) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long long *S = reinterpret_cast<const long long *>(G);
    const double mu = raw ? 1.0 : mean[0];
    for (int cc = ty; cc < 32; cc += 8) {
        const int r = tr * 32 + tx, c = tc * 32 + cc;
        double v = 0.0;
        if (r < n && c < n && r <= c) {
            v = grm_raw(S[(int64_t)c * ldG + r], a[r], a[c], nd, cn2);
            if (!raw) {
                v /= mu;
                if (r == c) v += lambda;
            }
        }
        tile[cc][tx] = v;
    }
    __syncthreads();
    for (int cc = ty; cc < 32; cc += 8) {
        const int r = tr * 32 + tx, c = tc * 32 + cc;
        if (r < n && c < n) G[(int64_t)c * ldG + r] = (r <= c) ? tile[cc][tx] : tile[tx][cc];
    }
    if (tr == tc) return;
    for (int cc = ty; cc < 32; cc += 8) {
        const int r = tc * 32 + tx, c = tr * 32 + cc; // the mirrored tile: entry (r, c) = entry (c, r) of the computed one
        if (r < n && c < n) G[(int64_t)c * ldG + r] = tile[tx][cc];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// polygenic block
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int PT = 256;

__device__ __forceinline__ d2 ld_p(const d2 *__restrict__ a, const d2 *__restrict__ b, int k)
{
    d2 p = a[k];
    if (b) p += b[k];
    return p;
}

struct poly_epi {
    const double *Kval;
    double *o0, *o1, *o2;   // mode 0: t, w, ev | mode 1: Kg, qt | mode 2: out
    const double *st;       // mode 0: the device's vb
    double vare, vb_in, sumvx;
    uint64_t seed, sub;
};

// out_j = K[:, j] . (a + b), a wave per column (b may be NULL). 16-byte non-temporal loads of the column — it is read once per pass and
// the matrix is far larger than L2 —, four independent ones in flight per lane, the vector through the cache. ld is even and K, a, b are
// 16-byte aligned, so every pair is; an odd n leaves one element, which lane 0 adds.
template <int MODE> __global__ __launch_bounds__(PT) void k_poly_dot(const double *__restrict__ K, int64_t ld, int n, const double *__restrict__ a,
                                                                     const double *__restrict__ b, poly_epi e)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = blockIdx.x * (PT / 64) + wave;
    if (j >= n) return; // (uniform in the wave)
    const double *col = K + (int64_t)j * ld;
    const d2 *c2 = reinterpret_cast<const d2 *>(col), *a2 = reinterpret_cast<const d2 *>(a), *b2 = reinterpret_cast<const d2 *>(b);
    const int n2 = n >> 1;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int k = lane;
    for (; k + 192 < n2; k += 256) {
        const d2 v0 = __builtin_nontemporal_load(c2 + k), v1 = __builtin_nontemporal_load(c2 + k + 64);
        const d2 v2 = __builtin_nontemporal_load(c2 + k + 128), v3 = __builtin_nontemporal_load(c2 + k + 192);
        const d2 q0 = ld_p(a2, b2, k), q1 = ld_p(a2, b2, k + 64), q2 = ld_p(a2, b2, k + 128), q3 = ld_p(a2, b2, k + 192);
        s0 = fma(v0.y, q0.y, fma(v0.x, q0.x, s0));
        s1 = fma(v1.y, q1.y, fma(v1.x, q1.x, s1));
        s2 = fma(v2.y, q2.y, fma(v2.x, q2.x, s2));
        s3 = fma(v3.y, q3.y, fma(v3.x, q3.x, s3));
    }
    for (; k < n2; k += 64) {
        const d2 v = __builtin_nontemporal_load(c2 + k), q = ld_p(a2, b2, k);
        s0 = fma(v.y, q.y, fma(v.x, q.x, s0));
    }
    double s = (s0 + s1) + (s2 + s3);
    if (lane == 0 && (n & 1)) s = fma(col[n - 1], a[n - 1] + (b ? b[n - 1] : 0.0), s);
    s = wave_sum(s);
    if (lane != 0) return;
    const double kv = e.Kval[j];
    if (MODE == 0) {
        const double vb = e.vb_in >= 0.0 ? e.vb_in : e.st[0];
        const double eval = (kv * e.vare) / (kv + e.vare / vb);                 // :531
        const double z = hb_normal_blk(e.seed, e.sub, (uint64_t)j);
        e.o0[j] = s;
        e.o1[j] = (eval / e.vare) * s + sqrt(fmax(eval, 0.0)) * z;              // :532, :534-535 as one vector
        e.o2[j] = eval;
    } else if (MODE == 1) {
        e.o0[j] = s;
        e.o1[j] = s * s / kv;                                                    // :544
    } else {
        e.o0[j] = s / kv / e.sumvx;                                              // :958-959
    }
}

// parts[chunk][row] = sum over the chunk's columns j, in order, of K[row][j] w[j]; a lane owns rows 2 rp, 2 rp + 1
__global__ __launch_bounds__(PT) void k_poly_kw(const double *__restrict__ K, int64_t ld, int n, const double *__restrict__ w, int cpc, double *__restrict__ parts)
{
    const int rp = blockIdx.x * PT + threadIdx.x;
    if (2 * rp >= n) return;
    const int c0 = blockIdx.y * cpc, c1 = min(n, c0 + cpc);
    const d2 *p = reinterpret_cast<const d2 *>(K + (int64_t)c0 * ld) + rp;
    const int64_t st = ld >> 1;
    d2 acc = {0.0, 0.0};
    int j = c0;
    for (; j + 3 < c1; j += 4, p += 4 * st) {
        const d2 v0 = __builtin_nontemporal_load(p), v1 = __builtin_nontemporal_load(p + st);
        const d2 v2 = __builtin_nontemporal_load(p + 2 * st), v3 = __builtin_nontemporal_load(p + 3 * st);
        const double w0 = w[j], w1 = w[j + 1], w2 = w[j + 2], w3 = w[j + 3];
        acc.x = fma(v0.x, w0, acc.x); acc.y = fma(v0.y, w0, acc.y);
        acc.x = fma(v1.x, w1, acc.x); acc.y = fma(v1.y, w1, acc.y);
        acc.x = fma(v2.x, w2, acc.x); acc.y = fma(v2.y, w2, acc.y);
        acc.x = fma(v3.x, w3, acc.x); acc.y = fma(v3.y, w3, acc.y);
    }
    for (; j < c1; j++, p += st) {
        const d2 v = __builtin_nontemporal_load(p);
        const double wj = w[j];
        acc.x = fma(v.x, wj, acc.x); acc.y = fma(v.y, wj, acc.y);
    }
    *(reinterpret_cast<d2 *>(parts + (int64_t)blockIdx.y * ld) + rp) = acc;
}

// k_new[i] = the chunks' partials in chunk order. update != 0: the residual update of :537-540 with k_cur the block's state; else out = k_new
__global__ __launch_bounds__(PT) void k_poly_fold(const double *__restrict__ parts, int nchunk, int64_t ld, int n, double *__restrict__ k_cur,
                                                  double *__restrict__ r, float *__restrict__ r32, double *__restrict__ u, double *__restrict__ out, int update)
{
    const int i = blockIdx.x * PT + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int c = 0; c < nchunk; c++) s += parts[(int64_t)c * ld + i];
    if (!update) {
        out[i] = s;
        return;
    }
    const double d = k_cur[i] - s;
    const double v = r[i] + d;
    r[i] = v;
    r32[i] = (float)v;
    u[i] -= d;
    k_cur[i] = s;
}

// one workgroup: q = sum_j qt[j] (thread t adds qt[t], qt[t + 256], ... in order, the 256 partials in a fixed tree), the check of :533, vb
__global__ __launch_bounds__(PT) void k_poly_final(const double *__restrict__ qt, const double *__restrict__ ev, int n, double s2_df, double chis,
                                                   double *__restrict__ st)
{
    __shared__ double red[PT], rmin[PT], rmax[PT];
    __shared__ int rbad[PT];
    double s = 0.0, lo = INFINITY, hi = 0.0;
    int bad = 0;
    for (int j = threadIdx.x; j < n; j += PT) {
        s += qt[j];
        const double e = ev[j];
        bad |= (e != e);
        lo = fmin(lo, e);
        hi = fmax(hi, fabs(e));
    }
    red[threadIdx.x] = s; rmin[threadIdx.x] = lo; rmax[threadIdx.x] = hi; rbad[threadIdx.x] = bad;
    __syncthreads();
    for (int o = PT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[threadIdx.x] += red[threadIdx.x + o];
            rmin[threadIdx.x] = fmin(rmin[threadIdx.x], rmin[threadIdx.x + o]);
            rmax[threadIdx.x] = fmax(rmax[threadIdx.x], rmax[threadIdx.x + o]);
            rbad[threadIdx.x] |= rbad[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        st[0] = (red[0] + s2_df) / chis;
        st[1] = red[0];
        st[2] = (rbad[0] || !(rmin[0] >= -1e-06 * rmax[0])) ? 1.0 : 0.0; // all(eval >= -1e-06 * max(abs(eval)))
    }
}

__global__ __launch_bounds__(PT) void k_poly_axpy(double *__restrict__ y, const double *__restrict__ x, int n, double a)
{
    const int i = blockIdx.x * PT + threadIdx.x;
    if (i < n) y[i] = fma(a, x[i], y[i]);
}

int poly_check(hb_ctx *c, const char *who)
{
    if (!c) return hb_fail(HB_ERR_INVALID, std::string(who) + ": null context");
    if (!c->poly) return hb_fail(HB_ERR_INVALID, std::string(who) + ": call hb_ctx_poly_setup first");
    HB_HIP(hipSetDevice(c->device));
    return HB_OK;
}

template <int MODE> int poly_dot(hb_ctx *c, const double *a, const double *b, const poly_epi &e)
{
    const hb_poly *p = c->poly;
    hipLaunchKernelGGL(k_poly_dot<MODE>, dim3((unsigned)((p->n + PT / 64 - 1) / (PT / 64))), dim3(PT), 0, c->stream, p->K, p->ld, p->n, a, b, e);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

// parts = the chunks' partial sums of K w
int poly_kw(hb_ctx *c, const double *w)
{
    const hb_poly *p = c->poly;
    const int rp = (p->n + 1) / 2;
    hipLaunchKernelGGL(k_poly_kw, dim3((unsigned)((rp + PT - 1) / PT), (unsigned)p->nchunk), dim3(PT), 0, c->stream, p->K, p->ld, p->n, w, p->cpc, p->parts);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

} // namespace

void hb_poly_free(hb_ctx *c)
{
    hb_poly *p = c ? c->poly : nullptr;
    if (!p) return;
    delete p;
    c->poly = nullptr;
}

// vb, q and the flag ride on the sweep's fetch (fetch_acc, hb_ctx.hip): no host synchronisation of their own
int hb_poly_fetch_enqueue(hb_ctx *c)
{
    hb_poly *p = c->poly;
    if (!p) return HB_OK;
    HB_HIP(hipMemcpyAsync(p->h_st, p->st, sizeof(double) * 4, hipMemcpyDeviceToHost, c->stream));
    return HB_OK;
}

const double *hb_poly_host_state(const hb_ctx *c) { return c && c->poly ? c->poly->h_st : nullptr; }

int hb_poly_reset(hb_ctx *c)
{
    int rc = poly_check(c, "hb_poly_reset");
    if (rc) return rc;
    hb_poly *p = c->poly;
    const size_t vl = sizeof(double) * (size_t)(p->ld + 2);
    HB_HIP(hipMemsetAsync(p->k_cur, 0, vl, c->stream));
    HB_HIP(hipMemsetAsync(p->k_sum, 0, vl, c->stream));
    HB_HIP(hipMemsetAsync(p->st, 0, sizeof(double) * 4, c->stream));
    p->stored = 0;
    return HB_OK;
}

// k_sum += k (the thinned store of :858)
int hbk_poly_accumulate(hb_ctx *c)
{
    int rc = poly_check(c, "hbk_poly_accumulate");
    if (rc) return rc;
    hb_poly *p = c->poly;
    hipLaunchKernelGGL(k_poly_axpy, dim3((unsigned)((p->n + PT - 1) / PT)), dim3(PT), 0, c->stream, p->k_sum, p->k_cur, p->n, 1.0);
    HB_HIP(hipGetLastError());
    p->stored++;
    return HB_OK;
}

// :956-961 up to the product with X': k_mean = k_sum / count and v = K ((K' k_mean) / Kval / sumvx), both to the host (n each)
int hbk_poly_backproject(hb_ctx *c, double sumvx, int count, double *k_mean, double *v)
{
    int rc = poly_check(c, "hbk_poly_backproject");
    if (rc) return rc;
    hb_poly *p = c->poly;
    const int n = p->n;
    HB_HIP(hipMemsetAsync(p->vec, 0, sizeof(double) * (size_t)(p->ld + 2), c->stream));
    hipLaunchKernelGGL(k_poly_axpy, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0, c->stream, p->vec, p->k_sum, n, 1.0 / (double)std::max(1, count));
    HB_HIP(hipGetLastError());
    poly_epi e{};
    e.Kval = p->Kval;
    e.o0 = p->Kg;
    e.sumvx = sumvx;
    rc = poly_dot<2>(c, p->vec, nullptr, e);
    if (!rc) rc = poly_kw(c, p->Kg);
    if (rc) return rc;
    HB_HIP(hipMemcpyAsync(k_mean, p->vec, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    hipLaunchKernelGGL(k_poly_fold, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0, c->stream, p->parts, p->nchunk, p->ld, n, nullptr, nullptr, nullptr, nullptr,
                       p->vec, 0);
    HB_HIP(hipGetLastError());
    HB_HIP(hipMemcpyAsync(v, p->vec, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    return HB_OK;
}

extern "C" {

int hb_grm_build(hb_ctx *c, double lambda, int32_t flags, double *G_host, double **G_dev)
{
    if (G_dev) *G_dev = nullptr;
    if (!c) return hb_fail(HB_ERR_INVALID, "hb_grm_build: null context");
    if (flags & ~HB_GRM_RAW) return hb_fail(HB_ERR_INVALID, "hb_grm_build: unknown flag");
    if (!G_host && !G_dev) return hb_fail(HB_ERR_INVALID, "hb_grm_build: nowhere to put the matrix (G_host and G_dev are NULL)");
    if (!std::isfinite(lambda)) return hb_fail(HB_ERR_INVALID, "hb_grm_build: lambda must be finite");
    HB_HIP(hipSetDevice(c->device));
    if (c->layout == 64)
        return hb_fail(HB_ERR_UNSUPPORTED, "hb_grm_build: the context holds the fp64 resident layout (real-valued genotypes); the relationship matrix is an integer contraction");
    if (!c->X) return hb_fail(HB_ERR_INVALID, "hb_grm_build: the context holds its genotypes in the 2-bit layout only (hb_ctx_set_layout(c, 8, 1) unpacks them)");
    int rc;
    if (!c->stats_ready) {
        rc = hbk_stats(c);
        if (rc) return rc;
    }
    const int n = c->n, m = c->m, raw = (flags & HB_GRM_RAW) ? 1 : 0;
    const double nd = (double)n;
    // C = sum_k c_k^2 in 128-bit integers (c_k^2 m can pass 2^63 for int8-coded genotypes), cn2 = (double)C / (n n): both roundings to nearest
    std::vector<double> s1(m);
    HB_HIP(hipMemcpyAsync(s1.data(), c->s1, sizeof(double) * m, hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    unsigned __int128 C = 0;
    for (int k = 0; k < m; k++) {
        const long long ck = (long long)s1[k];
        C += (unsigned __int128)((__int128)ck * ck);
    }
    const double cn2 = (double)C / (nd * nd);

    hb_bufs mem;
    struct { double *G = nullptr, *d = nullptr; long long *a = nullptr; } B;
    HB_TRY(mem.big(&B.G, (size_t)n * (size_t)n, "hb_grm_build", "the " + hb_dims(n) + " matrix"));
    HB_TRY(mem.get(&B.d, (size_t)(n + 1)));
    HB_TRY(mem.zeroed(&B.a, (size_t)n, c->stream));
    long long *S = reinterpret_cast<long long *>(B.G);
    const int nt = (n + GT - 1) / GT;
    const unsigned ntri = (unsigned)((long long)nt * (nt + 1) / 2);
    for (int k0 = 0; k0 < m; k0 += GRM_KCHUNK) {
        hipLaunchKernelGGL(k_grm_tile, dim3(ntri), dim3(256), 0, c->stream, c->X, c->ld, n, k0, std::min(m, k0 + GRM_KCHUNK), S, (int64_t)n, k0 == 0 ? 1 : 0);
        HB_HIP(hipGetLastError());
    }
    {
        const int rowblocks = (n + 255) / 256;
        const int nks = std::max(1, std::min((m + 255) / 256, 2048 / rowblocks));
        const int kslice = (m + nks - 1) / nks;
        hipLaunchKernelGGL(k_grm_a, dim3((unsigned)rowblocks, (unsigned)((m + kslice - 1) / kslice)), dim3(256), 0, c->stream, c->X, c->ld, n, m, kslice, c->s1,
                           reinterpret_cast<unsigned long long *>(B.a));
        HB_HIP(hipGetLastError());
    }
    double mean = 1.0;
    if (!raw) {
        hipLaunchKernelGGL(k_grm_diag, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, S, (int64_t)n, n, B.a, nd, cn2, B.d);
        hipLaunchKernelGGL(k_grm_mean, dim3(1), dim3(256), 0, c->stream, B.d, n, B.d + n);
        HB_HIP(hipGetLastError());
        HB_HIP(hipMemcpyAsync(&mean, B.d + n, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        if (!(mean > 0.0))
            return hb_fail(HB_ERR_INVALID, "make_grm: the mean diagonal of Z Z' is 0 — every marker is monomorphic, there is no relationship matrix to scale");
    }
    const unsigned nt32 = (unsigned)((n + 31) / 32);
    hipLaunchKernelGGL(k_grm_combine, dim3(nt32, nt32), dim3(256), 0, c->stream, B.G, (int64_t)n, n, B.a, nd, cn2, B.d + n, lambda, raw);
    HB_HIP(hipGetLastError());
    if (G_host) HB_HIP(hipMemcpyAsync(G_host, B.G, sizeof(double) * (size_t)n * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    if (G_dev) {
        *G_dev = B.G;
        mem.release(B.G); // the caller's from here (hb_grm_free)
    }
    return HB_OK;
}

void hb_grm_free(double *G_dev)
{
    hb_free_released(G_dev);
}

int hb_ctx_poly_setup(hb_ctx *c, const double *Kival, const double *Ki, int64_t ld, int32_t on_device)
{
    if (!c) return hb_fail(HB_ERR_INVALID, "hb_ctx_poly_setup: null context");
    HB_HIP(hipSetDevice(c->device));
    if (c->stream) HB_HIP(hipStreamSynchronize(c->stream));
    hb_poly_free(c);
    if (!Kival && !Ki) return HB_OK; // (drops the block)
    if (!Kival || !Ki) return hb_fail(HB_ERR_INVALID, "hb_ctx_poly_setup: Kival and Ki go together");
    const int n = c->n;
    if (ld < n) return hb_fail(HB_ERR_INVALID, "hb_ctx_poly_setup: leading dimension smaller than the number of individuals");
    if (on_device && ((ld & 1) || (reinterpret_cast<uintptr_t>(Ki) & 15u)))
        return hb_fail(HB_ERR_INVALID, "hb_ctx_poly_setup: a device matrix must be 16-byte aligned with an even leading dimension");
    for (int j = 0; j < n; j++)
        if (std::isnan(Kival[j])) return hb_fail(HB_ERR_INVALID, "hb_ctx_poly_setup: NaN in Kival");
    hb_poly *p = new hb_poly();
    c->poly = p;
    p->n = n;
    p->ld = on_device ? ld : (int64_t)n + (n & 1);
    auto build = [&]() -> int {
        if (on_device) p->K = Ki;
        else {
            HB_TRY(p->mem.big(&p->K_own, (size_t)p->ld * (size_t)n, "hb_ctx_poly_setup", "the " + hb_dims(n) + " eigenvector matrix"));
            if (p->ld != n) HB_HIP(hipMemsetAsync(p->K_own, 0, sizeof(double) * (size_t)p->ld * (size_t)n, nullptr));
            HB_HIP(hipMemcpy2D(p->K_own, sizeof(double) * (size_t)p->ld, Ki, sizeof(double) * (size_t)ld, sizeof(double) * (size_t)n, (size_t)n, hipMemcpyHostToDevice));
            p->K = p->K_own;
        }
        // chunks of k_poly_kw: a function of n alone (the summation order must not depend on the device), about 2048 workgroups, chunks of >= 64 columns
        const int rowblocks = ((n + 1) / 2 + PT - 1) / PT;
        const int want = std::max(1, 2048 / rowblocks);
        p->cpc = std::max(64, (n + want - 1) / want);
        p->nchunk = (n + p->cpc - 1) / p->cpc;
        // (zeroed on the null stream, like the copy of Kval behind them: that copy returns after them)
        double **vecs[] = {&p->Kval, &p->k_cur, &p->k_sum, &p->t, &p->w, &p->ev, &p->Kg, &p->qt, &p->vec};
        for (double **v : vecs) HB_TRY(p->mem.zeroed(v, (size_t)(p->ld + 2), nullptr));
        HB_TRY(p->mem.zeroed(&p->parts, (size_t)p->ld * (size_t)p->nchunk, nullptr));
        HB_TRY(p->mem.zeroed(&p->st, 4, nullptr));
        HB_TRY(p->mem.pin(&p->h_st, 4));
        std::memset(p->h_st, 0, sizeof(double) * 4);
        HB_HIP(hipMemcpy(p->Kval, Kival, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
        return HB_OK;
    };
    const int rc = build();
    if (rc) hb_poly_free(c);
    return rc;
}

int hb_ctx_poly_step(hb_ctx *c, double vare, double vb_in, uint64_t seed, int64_t iter, double chis, double s2_df)
{
    int rc = poly_check(c, "hb_ctx_poly_step");
    if (rc) return rc;
    hb_poly *p = c->poly;
    const int n = p->n;
    poly_epi e{};
    e.Kval = p->Kval;
    e.o0 = p->t;
    e.o1 = p->w;
    e.o2 = p->ev;
    e.st = p->st;
    e.vare = vare;
    e.vb_in = vb_in;
    e.seed = seed;
    e.sub = hb_sub(HB_PURPOSE_POLY, (uint64_t)iter);
    rc = poly_dot<0>(c, c->r, p->k_cur, e);        // t = K'(yadj + k_old), w
    if (!rc) rc = poly_kw(c, p->w);                // partials of K w
    if (rc) return rc;
    hipLaunchKernelGGL(k_poly_fold, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0, c->stream, p->parts, p->nchunk, p->ld, n, p->k_cur, c->r, c->r32, c->u,
                       nullptr, 1);
    HB_HIP(hipGetLastError());
    poly_epi e1{};
    e1.Kval = p->Kval;
    e1.o0 = p->Kg;
    e1.o1 = p->qt;
    rc = poly_dot<1>(c, p->k_cur, nullptr, e1);    // Kg = K' k_new
    if (rc) return rc;
    hipLaunchKernelGGL(k_poly_final, dim3(1), dim3(PT), 0, c->stream, p->qt, p->ev, n, s2_df, chis, p->st);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hb_ctx_poly_state(hb_ctx *c, double *k, double *vb, double *q, int32_t *flag)
{
    int rc = poly_check(c, "hb_ctx_poly_state");
    if (rc) return rc;
    hb_poly *p = c->poly;
    rc = hb_poly_fetch_enqueue(c);
    if (rc) return rc;
    if (k) HB_HIP(hipMemcpyAsync(k, p->k_cur, sizeof(double) * (size_t)p->n, hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    if (vb) *vb = p->h_st[0];
    if (q) *q = p->h_st[1];
    if (flag) *flag = p->h_st[2] != 0.0;
    return HB_OK;
}

int hb_ctx_poly_debug_get(hb_ctx *c, double *t, double *w, double *eval, double *Kg)
{
    int rc = poly_check(c, "hb_ctx_poly_debug_get");
    if (rc) return rc;
    hb_poly *p = c->poly;
    HB_HIP(hipStreamSynchronize(c->stream));
    const size_t nb = sizeof(double) * (size_t)p->n;
    if (t) HB_HIP(hipMemcpy(t, p->t, nb, hipMemcpyDeviceToHost));
    if (w) HB_HIP(hipMemcpy(w, p->w, nb, hipMemcpyDeviceToHost));
    if (eval) HB_HIP(hipMemcpy(eval, p->ev, nb, hipMemcpyDeviceToHost));
    if (Kg) HB_HIP(hipMemcpy(Kg, p->Kg, nb, hipMemcpyDeviceToHost));
    return HB_OK;
}

} // extern "C"
