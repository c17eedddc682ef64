// hb_cg.hip — sbrm()'s method = "CG": the conjugate-gradient ridge solve (V + diag(lambda)) g = b of the reference (CG(),
// src/solver.cpp:54-115, called by conjgt_den / conjgt_spa, src/cg.cpp:4-129) on the device. A unit of its own: it shares
// nothing with the chain kernels' unit but hb_wave.hpp. DESIGN.md §14.
//
// The LD matrix is symmetric (hb_ldm_from_csc checks it, hb_ldm_build's are by construction, k_cg_symcheck checks a host dense
// matrix), so row i of V is column i: in the column-major dense matrix and in the CSC alike (V p)[i] is ONE contiguous dot
// product. No split-K, no floating-point atomic: every sum below is formed in one fixed order and two runs agree bit for bit.
//
// One iteration = three launches, the kernel boundary being the only grid-wide synchronisation:
//   k_cg_matvec_dense / k_cg_matvec_csc   ap = V p + lambda o p, and each workgroup's partial sum of p[i] ap[i]
//   k_cg_step1   every workgroup re-adds those partials in index order -> pAp; alpha = r2 / pAp; x += alpha p; r -= alpha ap;
//                leaves partials of r . r
//   k_cg_step2   r2update, err = sqrt(r2update) -> err_hist[i]; err < esp: the stop word; otherwise beta = r2update / r2 and
//                p = r + beta p
// r2 is not a stored scalar: the partials of r . r live in two halves indexed by the iteration's parity and whoever needs r2
// or r2update re-adds its half, so no workgroup reads a word that another workgroup of the same launch writes. The stop word
// holds the number of iterations run at the reference's `break` (0: none yet); a kernel of iteration i returns at once when it
// is in 1..i. The host enqueues iterations in chunks and looks at the word once per chunk (cg_run).
#include "hb_internal.hpp"
#include "hb_ldm.hpp"
#include "hb_model.hpp"
#include "hb_wave.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace {
constexpr int CG_T = 256;            // threads per workgroup, every kernel of this unit
constexpr int CG_W = CG_T / 64;      // waves per workgroup = dense columns per workgroup

// workgroup-wide sum in a fixed order, the result in every thread; red holds CG_W entries. Not hb_wave.hpp's block_sum: this one
// is for CG_W = 4 waves alone and starts from r0, not from 0 + r0 (a sum of negative zeros keeps its sign), and the unit's
// bit-for-bit tests rest on the sums it gives today.
__device__ __forceinline__ double block_sum(double v, double *red)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// the sum of n partials, the same order in every workgroup that forms it
__device__ __forceinline__ double sum_parts(const double *__restrict__ parts, int n, double *red)
{
    double s = 0.0;
    for (int k = threadIdx.x; k < n; k += CG_T) s += parts[k];
    return block_sum(s, red);
}

// has the solve stopped before iteration `it`?
__device__ __forceinline__ bool cg_stopped(const int *stop, int it)
{
    if (!stop) return false;
    const int s = *stop;
    return s != 0 && s <= it;
}

// p[2k + off], p[2k + off + 1] from the 16-byte pairs P of p: the pair itself (off = 0), or the halves of two neighbouring
// pairs (off = 1) — two aligned loads that hit the cache instead of one that straddles a 16-byte boundary. P[k + 1] may reach
// one pair past p[m - 1]: cg_run allocates the vectors with that pair.
template <bool PAL> __device__ __forceinline__ d2 load_p(const d2 *__restrict__ P, int k)
{
    if (PAL) return P[k];
    const d2 a = P[k], b = P[k + 1];
    d2 q;
    q.x = a.y;
    q.y = b.x;
    return q;
}

// sum over pairs k = lane, lane + 64, ... < n2 of c2[k] . load_p(k): 16-byte non-temporal loads of the column (it is
// read once per iteration and is far larger than L2), four independent ones in flight per lane, p through the cache
template <bool PAL> __device__ __forceinline__ double dot_pairs(const d2 *__restrict__ c2, const d2 *__restrict__ p, int n2, int lane)
{
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int k = lane;
    for (; k + 192 < n2; k += 256) {
        const d2 v0 = __builtin_nontemporal_load(c2 + k), v1 = __builtin_nontemporal_load(c2 + k + 64);
        const d2 v2 = __builtin_nontemporal_load(c2 + k + 128), v3 = __builtin_nontemporal_load(c2 + k + 192);
        const d2 q0 = load_p<PAL>(p, k), q1 = load_p<PAL>(p, k + 64), q2 = load_p<PAL>(p, k + 128), q3 = load_p<PAL>(p, k + 192);
        a0 = fma(v0.y, q0.y, fma(v0.x, q0.x, a0));
        a1 = fma(v1.y, q1.y, fma(v1.x, q1.x, a1));
        a2 = fma(v2.y, q2.y, fma(v2.x, q2.x, a2));
        a3 = fma(v3.y, q3.y, fma(v3.x, q3.x, a3));
    }
    for (; k < n2; k += 64) {
        const d2 v = __builtin_nontemporal_load(c2 + k), q = load_p<PAL>(p, k);
        a0 = fma(v.y, q.y, fma(v.x, q.x, a0));
    }
    return (a0 + a1) + (a2 + a3);
}

// ap = V p (+ lambda o p) on the column-major dense matrix, a wave per column (= row, by symmetry); parts[workgroup] = the sum
// of p[j] ap[j] over its CG_W columns. Column j starts at j * ld * 8 bytes: with an odd ld every other column is only 8-byte
// aligned, so the element in front of the first 16-byte boundary is peeled (lane 0) and p is then taken from two aligned pairs.
// CONTRACT: p is 16-byte aligned and has m + 2 doubles allocated — the odd-alignment path reads (and discards) the pair behind
// p[m - 1]; cg_mat::launch refuses an operand that is shorter.
__global__ __launch_bounds__(CG_T) void k_cg_matvec_dense(const double *__restrict__ V, int64_t ld, int m, const double *__restrict__ p,
                                                          const double *__restrict__ lambda, double *__restrict__ ap,
                                                          double *__restrict__ parts, const int *stop, int it)
{
    __shared__ double red[CG_W];
    if (cg_stopped(stop, it)) return; // (uniform)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = blockIdx.x * CG_W + wave;
    double c = 0.0;
    if (j < m) { // (uniform in the wave)
        const double *col = V + (size_t)j * (size_t)ld;
        const int off = (int)((reinterpret_cast<uintptr_t>(col) >> 3) & 1u);
        const int n2 = (m - off) >> 1, tail = off + 2 * n2;
        const d2 *c2 = reinterpret_cast<const d2 *>(col + off);
        const d2 *P = reinterpret_cast<const d2 *>(p); // (p is a whole allocation: 16-byte aligned)
        double s = off ? dot_pairs<false>(c2, P, n2, lane) : dot_pairs<true>(c2, P, n2, lane);
        if (lane == 0) {
            if (off) s = fma(col[0], p[0], s);
            if (tail < m) s = fma(col[tail], p[tail], s);
        }
        s = wave_sum(s);
        const double pj = p[j];
        if (lambda) s = fma(lambda[j], pj, s);
        if (lane == 0) ap[j] = s;
        c = pj * s;
    }
    if (lane == 0) red[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) parts[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// the same product from the device CSC, column j read as row j; LPC lanes walk a column (4, 16 or 64, chosen once per run from
// the mean number of stored entries per column), an empty column gives ap[j] = lambda[j] p[j]
template <int LPC>
__global__ __launch_bounds__(CG_T) void k_cg_matvec_csc(const int64_t *__restrict__ cp, const int32_t *__restrict__ ri, const double *__restrict__ va,
                                                        int m, const double *__restrict__ p, const double *__restrict__ lambda,
                                                        double *__restrict__ ap, double *__restrict__ parts, const int *stop, int it)
{
    __shared__ double red[CG_W];
    if (cg_stopped(stop, it)) return; // (uniform)
    const int l = threadIdx.x % LPC;
    const int j = blockIdx.x * (CG_T / LPC) + threadIdx.x / LPC;
    double s = 0.0;
    if (j < m) {
        const int64_t end = cp[j + 1];
#pragma unroll 4
        for (int64_t e = cp[j] + l; e < end; e += LPC) s = fma(va[e], p[ri[e]], s);
    }
#pragma unroll
    for (int o = LPC / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    double c = 0.0;
    if (j < m && l == 0) {
        const double pj = p[j];
        if (lambda) s = fma(lambda[j], pj, s);
        ap[j] = s;
        c = pj * s;
    }
    c = block_sum(c, red);
    if (threadIdx.x == 0) parts[blockIdx.x] = c;
}

// x = 0, r = b - A x - x o lambda = b (- 0 * lambda), p = r (src/solver.cpp:72-83); partials of r . r into half 0
__global__ __launch_bounds__(CG_T) void k_cg_init(int m, const double *__restrict__ b, const double *__restrict__ lambda, double *__restrict__ x,
                                                  double *__restrict__ r, double *__restrict__ p, double *__restrict__ rr)
{
    __shared__ double red[CG_W];
    const int j = blockIdx.x * CG_T + threadIdx.x;
    double c = 0.0;
    if (j < m) {
        double rj = b[j];
        if (lambda) rj -= 0.0 * lambda[j];
        x[j] = 0.0;
        r[j] = rj;
        p[j] = rj;
        c = rj * rj;
    }
    c = block_sum(c, red);
    if (threadIdx.x == 0) rr[blockIdx.x] = c;
}

// :93-95. rr: two halves of nb partials of r . r, the half of iteration `it`'s parity holds r2
__global__ __launch_bounds__(CG_T) void k_cg_step1(int it, int m, int na, const double *__restrict__ pap, int nb, double *__restrict__ rr,
                                                   const double *__restrict__ p, const double *__restrict__ ap, double *__restrict__ x,
                                                   double *__restrict__ r, const int *stop)
{
    __shared__ double red[CG_W];
    if (cg_stopped(stop, it)) return; // (uniform)
    const double pAp = sum_parts(pap, na, red);
    const double r2 = sum_parts(rr + (size_t)(it & 1) * nb, nb, red);
    const double alpha = r2 / pAp;
    const int j = blockIdx.x * CG_T + threadIdx.x;
    double c = 0.0;
    if (j < m) {
        x[j] = fma(alpha, p[j], x[j]);
        const double rj = fma(-alpha, ap[j], r[j]);
        r[j] = rj;
        c = rj * rj;
    }
    c = block_sum(c, red);
    if (threadIdx.x == 0) rr[(size_t)((it + 1) & 1) * nb + blockIdx.x] = c;
}

// :96-107
__global__ __launch_bounds__(CG_T) void k_cg_step2(int it, int m, int nb, const double *__restrict__ rr, double esp, const double *__restrict__ r,
                                                   double *__restrict__ p, double *__restrict__ err_hist, int *stop)
{
    __shared__ double red[CG_W];
    if (cg_stopped(stop, it)) return; // (uniform; a word written by this very launch is it + 1 and does not count)
    const double r2update = sum_parts(rr + (size_t)((it + 1) & 1) * nb, nb, red);
    const double err = sqrt(r2update);
    const bool brk = err < esp;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        err_hist[it] = err;
        if (brk) *stop = it + 1;
    }
    if (brk) return;
    const double r2 = sum_parts(rr + (size_t)(it & 1) * nb, nb, red);
    const double beta = r2update / r2;
    const int j = blockIdx.x * CG_T + threadIdx.x;
    if (j < m) p[j] = fma(beta, p[j], r[j]);
}

// one workgroup: out[0] = the sum of n partials (g' V g after the last mat-vec)
__global__ __launch_bounds__(CG_T) void k_cg_sum(const double *__restrict__ parts, int n, double *__restrict__ out)
{
    __shared__ double red[CG_W];
    const double s = sum_parts(parts, n, red);
    if (threadIdx.x == 0) out[0] = s;
}

// V[i][j] against V[j][i] bit for bit, 32 x 32 tiles of the upper block triangle, both tiles read along their columns;
// first = the smallest j * m + i (column-major position, i <= j up to the tile) of a pair that differs
__global__ __launch_bounds__(256) void k_cg_symcheck(const double *__restrict__ V, int64_t ld, int m, unsigned long long *first)
{
    __shared__ unsigned long long A[32][33], B[32][33];
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bi > bj) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const unsigned long long *W = reinterpret_cast<const unsigned long long *>(V);
    for (int c = ty; c < 32; c += 8) {
        const int ra = bi * 32 + tx, ca = bj * 32 + c, rb = bj * 32 + tx, cb = bi * 32 + c;
        A[c][tx] = (ra < m && ca < m) ? W[(size_t)ca * (size_t)ld + ra] : 0ull;
        B[c][tx] = (rb < m && cb < m) ? W[(size_t)cb * (size_t)ld + rb] : 0ull;
    }
    __syncthreads();
    for (int c = ty; c < 32; c += 8) {
        const int row = bi * 32 + tx, col = bj * 32 + c;
        if (row < m && col < m && A[c][tx] != B[tx][c]) atomicMin(first, (unsigned long long)col * (unsigned long long)m + (unsigned long long)row);
    }
}

struct cg_dev {
    hipStream_t stream = nullptr;
    hb_bufs mem;
    int *h_stop = nullptr;
    double *h_err = nullptr;
    ~cg_dev()
    {
        if (stream) (void)hipStreamSynchronize(stream);
        mem.clear();
        if (stream) (void)hipStreamDestroy(stream);
    }
    template <typename T> int alloc(T **q, size_t count) { return mem.zeroed(q, count, stream); }
};

// what one run's mat-vec reads: the dense matrix or the CSC
struct cg_mat {
    const double *V = nullptr;
    int64_t ld = 0;
    hb_ldm_csc csc{};
    int lpc = 0; // 0: dense; 4 / 16 / 64 lanes per column of the CSC
    int m = 0;
    int blocks() const { return lpc ? (m + CG_T / lpc - 1) / (CG_T / lpc) : (m + CG_W - 1) / CG_W; }
    // p_len: the doubles allocated behind p. The dense kernel's contract (load_p): p is a whole 16-byte aligned allocation
    // with one pair of slack behind p[m - 1].
    int launch(hipStream_t s, const double *p, size_t p_len, const double *lambda, double *ap, double *parts, const int *stop, int it) const
    {
        if (!lpc && (p_len < (size_t)m + 2 || (reinterpret_cast<uintptr_t>(p) & 15u)))
            return hb_fail(HB_ERR_INVALID, "hb_cg: the dense mat-vec needs a 16-byte aligned operand of m + 2 doubles");
        const dim3 g((unsigned)blocks()), b(CG_T);
        if (!lpc) hipLaunchKernelGGL(k_cg_matvec_dense, g, b, 0, s, V, ld, m, p, lambda, ap, parts, stop, it);
        else if (lpc == 4) hipLaunchKernelGGL(k_cg_matvec_csc<4>, g, b, 0, s, csc.cp, csc.ri, csc.va, m, p, lambda, ap, parts, stop, it);
        else if (lpc == 16) hipLaunchKernelGGL(k_cg_matvec_csc<16>, g, b, 0, s, csc.cp, csc.ri, csc.va, m, p, lambda, ap, parts, stop, it);
        else hipLaunchKernelGGL(k_cg_matvec_csc<64>, g, b, 0, s, csc.cp, csc.ri, csc.va, m, p, lambda, ap, parts, stop, it);
        return HB_OK;
    }
};

// conjgt_den (H == nullptr: args->ldm on the host; H: the handle's dense device copy) and conjgt_spa (sparse: the handle's CSC)
int cg_run(const hb_cg_args *args, hb_ldm *H, hb_cg_out *o, bool sparse)
{
    if (!args || !o) return hb_fail(HB_ERR_INVALID, "hb_cg_run: null argument");
    const auto t_setup = hb_clk::now();
    const hb_cg_args &a = *args;
    const int m = a.m;
    if (H ? (m < 1 || !a.sumstat || a.ldm || a.ld_sumstat < m || H->m != m)
          : (m < 1 || !a.sumstat || !a.ldm || a.ld_sumstat < m || a.ld_ldm < m)) return hb_fail(HB_ERR_INVALID, "Number of SNPs not equals."); // src/cg.cpp:15-17, :79-81
    auto line = [&](const char *fmt, auto... xs) { hb_line(a.verbose, a.log, a.log_user, fmt, xs...); };
    // ---- src/cg.cpp:12-41, :77-103 ----
    const double *ss = a.sumstat;
    const int64_t lds = a.ld_sumstat;
    const int n = hb_sumstat_n(ss, lds, m); // :13 int n = mean(na_omit(NMISS))
    std::vector<double> xpx(m), b(m), yyi(m, 0.0);
    int count_y = 0;
    for (int k = 0; k < m; k++) {
        const double vx = H ? H->diag[k] : a.ldm[(size_t)k * (size_t)a.ld_ldm + k];
        const double be = ss[1 * lds + k], se = ss[2 * lds + k], N = ss[3 * lds + k];
        xpx[k] = vx * n;
        b[k] = xpx[k] * be / n; // :30 xy, :51 xy / n — a NaN BETA is not filtered
        if (!std::isnan(se)) {  // :31-36
            yyi[k] = xpx[k] * (be * be + (N - 2) * se * se);
            count_y++;
        }
    }
    if (count_y == 0) return hb_fail(HB_ERR_INVALID, "Lack of SE.");
    const double yy = arma_sum(yyi.data(), m) / count_y;
    const double vary = yy / (n - 1);

    // ---- device ----
    if (hb_device_count() <= 0) return hb_fail(HB_ERR_NO_DEVICE, "no HIP device available: the hibayes GPU engine has no CPU fallback");
    if (H && H->device != a.device) return hb_fail(HB_ERR_INVALID, "hb_cg_run: the LD matrix was built on another device");
    if (a.device < 0 || a.device >= hb_device_count()) return hb_fail(HB_ERR_INVALID, "hb_cg_run: no such device");
    HB_HIP(hipSetDevice(a.device));
    cg_dev D;
    HB_HIP(hipStreamCreateWithFlags(&D.stream, hipStreamNonBlocking));
    cg_mat M;
    M.m = m;
    if (sparse) { // adopted, not owned; nothing m x m exists on this route
        HB_TRY(hb_ldm_device_csc(H, &M.csc));
        const double mean = (double)M.csc.nnz / m;
        M.lpc = mean < 16.0 ? 4 : mean < 256.0 ? 16 : 64;
    } else if (H) {
        HB_TRY(hb_ldm_device_dense(H, &M.V));
        M.ld = m;
    } else { // uploaded without its padding rows: the run is then the handle's, bit for bit
        double *dv = nullptr;
        unsigned long long *d_first = nullptr, h_first = 0;
        HB_TRY(D.alloc(&dv, (size_t)m * m));
        HB_TRY(D.alloc(&d_first, 1));
        HB_HIP(hipMemcpy2DAsync(dv, sizeof(double) * m, a.ldm, sizeof(double) * a.ld_ldm, sizeof(double) * m, m, hipMemcpyHostToDevice, D.stream));
        HB_HIP(hipMemsetAsync(d_first, 0xff, sizeof(unsigned long long), D.stream));
        const unsigned nt = (unsigned)((m + 31) / 32);
        hipLaunchKernelGGL(k_cg_symcheck, dim3(nt, nt), dim3(256), 0, D.stream, dv, (int64_t)m, m, d_first);
        HB_HIP(hipGetLastError());
        HB_HIP(hipMemcpyAsync(&h_first, d_first, sizeof(h_first), hipMemcpyDeviceToHost, D.stream));
        HB_HIP(hipStreamSynchronize(D.stream));
        if (h_first != ~0ull) {
            const long long i = (long long)(h_first % (unsigned long long)m), j = (long long)(h_first / (unsigned long long)m);
            char buf[160];
            snprintf(buf, sizeof(buf), "hb_cg_run: the LD matrix must equal its transpose in value bits: ldm[%lld][%lld] differs from ldm[%lld][%lld]", i, j, j, i);
            return hb_fail(HB_ERR_INVALID, buf);
        }
        M.V = dv;
        M.ld = m;
    }
    const int na = M.blocks(), nb = (m + CG_T - 1) / CG_T;
    double *d_b, *d_lam = nullptr, *d_x, *d_r, *d_p, *d_ap, *d_pap, *d_rr, *d_err, *d_s;
    int *d_stop;
    HB_TRY(D.alloc(&d_b, m));
    const size_t vlen = (size_t)m + 2; // x and p are mat-vec operands: one pair of zeros behind the end (load_p, cg_mat::launch)
    HB_TRY(D.alloc(&d_x, vlen));
    HB_TRY(D.alloc(&d_r, m));
    HB_TRY(D.alloc(&d_p, vlen));
    HB_TRY(D.alloc(&d_ap, m));
    HB_TRY(D.alloc(&d_pap, na));
    HB_TRY(D.alloc(&d_rr, (size_t)2 * nb));
    HB_TRY(D.alloc(&d_err, m));
    HB_TRY(D.alloc(&d_s, 1));
    HB_TRY(D.alloc(&d_stop, 1));
    if (a.lambda) {
        HB_TRY(D.alloc(&d_lam, m));
        HB_HIP(hipMemcpyAsync(d_lam, a.lambda, sizeof(double) * m, hipMemcpyHostToDevice, D.stream));
    }
    HB_TRY(D.mem.pin(&D.h_stop, 1));
    HB_TRY(D.mem.pin(&D.h_err, m));
    HB_HIP(hipMemcpyAsync(d_b, b.data(), sizeof(double) * m, hipMemcpyHostToDevice, D.stream));
    hipLaunchKernelGGL(k_cg_init, dim3(nb), dim3(CG_T), 0, D.stream, m, d_b, d_lam, d_x, d_r, d_p, d_rr);
    HB_HIP(hipGetLastError());
    HB_HIP(hipStreamSynchronize(D.stream));
    o->n = n;
    o->count_y = count_y;
    const double setup_seconds = hb_since(t_setup);

    line("Prior parameters:");
    line("    Model fitted at [Conjugate Gradient]");
    line("    Maximum iteration number: %d", m);
    line("    Phenotypic var %.4f", vary);

    // ---- CG(), src/solver.cpp:88-113: iterations in chunks, one look at the stop word per chunk ----
    const auto t_loop = hb_clk::now();
    const int chunk = std::min(64, a.outfreq > 0 ? a.outfreq : 64);
    auto enqueue = [&](int it) -> int {
        const int e = M.launch(D.stream, d_p, vlen, d_lam, d_ap, d_pap, d_stop, it);
        if (e) return e;
        hipLaunchKernelGGL(k_cg_step1, dim3(nb), dim3(CG_T), 0, D.stream, it, m, na, d_pap, nb, d_rr, d_p, d_ap, d_x, d_r, d_stop);
        hipLaunchKernelGGL(k_cg_step2, dim3(nb), dim3(CG_T), 0, D.stream, it, m, nb, d_rr, a.esp, d_r, d_p, d_err, d_stop);
        return HB_OK;
    };
    auto iter_line = [&](int i, double err) {
        if (a.outfreq > 0 && (i + 1) % a.outfreq == 0) line("Iter No.%d, err = %.6f", i, err); // :98-101 (i, not i + 1)
    };
    int iterations = m, converged = 0;
    bool nan = false;
    for (int it0 = 0; it0 < m && !converged && !nan;) {
        const int c = std::min(chunk, m - it0);
        for (int k = 0; k < c; k++) HB_TRY(enqueue(it0 + k));
        HB_HIP(hipGetLastError());
        HB_HIP(hipMemcpyAsync(D.h_stop, d_stop, sizeof(int), hipMemcpyDeviceToHost, D.stream));
        HB_HIP(hipMemcpyAsync(D.h_err + it0, d_err + it0, sizeof(double) * c, hipMemcpyDeviceToHost, D.stream));
        HB_HIP(hipStreamSynchronize(D.stream));
        const int stop = *D.h_stop;
        const int ran = stop ? stop : it0 + c; // iterations run so far
        for (int i = it0; i < ran; i++) {
            iter_line(i, D.h_err[i]);
            nan = nan || std::isnan(D.h_err[i]);
        }
        if (a.interrupt && a.interrupt(a.interrupt_user)) return hb_fail(HB_ERR_INTERRUPT, "interrupted");
        it0 += c;
        if (stop) {
            converged = 1;
            iterations = stop;
        } else if (nan) {
            // nothing finite can follow: the reference runs on to m with alpha NaN, which makes x NaN everywhere one iteration
            // after err at the latest — that iteration is run if the chunk ended on the first NaN
            if (it0 < m) {
                HB_TRY(enqueue(it0));
                HB_HIP(hipGetLastError());
                HB_HIP(hipStreamSynchronize(D.stream));
            }
            for (int i = ran; i < m; i++) {
                D.h_err[i] = D.h_err[ran - 1];
                iter_line(i, D.h_err[i]);
            }
        }
    }
    const double loop_seconds = hb_since(t_loop);
    const double err = D.h_err[iterations - 1];
    line(converged ? "Convergence: YES" : "Convergence: NO[try to adjust lambda]"); // :109-113

    // ---- src/cg.cpp:52-53, :115-116: one more mat-vec, without lambda ----
    HB_TRY(M.launch(D.stream, d_x, vlen, nullptr, d_ap, d_pap, nullptr, 0));
    hipLaunchKernelGGL(k_cg_sum, dim3(1), dim3(CG_T), 0, D.stream, d_pap, na, d_s);
    HB_HIP(hipGetLastError());
    double gVg = 0.0;
    HB_HIP(hipMemcpyAsync(&gVg, d_s, sizeof(double), hipMemcpyDeviceToHost, D.stream));
    if (o->g) HB_HIP(hipMemcpyAsync(o->g, d_x, sizeof(double) * m, hipMemcpyDeviceToHost, D.stream));
    HB_HIP(hipStreamSynchronize(D.stream));
    o->vg = n * gVg / (n - 1);
    o->ve = vary - o->vg;
    o->iterations = iterations;
    o->converged = converged;
    o->err = err;
    if (o->err_hist) {
        std::memcpy(o->err_hist, D.h_err, sizeof(double) * iterations);
        std::fill(o->err_hist + iterations, o->err_hist + m, 0.0);
    }
    o->setup_seconds = setup_seconds;
    o->loop_seconds = loop_seconds;
    line("Prior parameters:");
    line("    Genetic var %.4f", o->vg);
    line("    Residual var %.4f", o->ve);
    return HB_OK;
}
} // namespace

extern "C" int hb_cg_run(const hb_cg_args *args, hb_cg_out *out) { return cg_run(args, nullptr, out, false); }

extern "C" int hb_cg_run_ldm(const hb_cg_args *args, hb_ldm *ldm, hb_cg_out *out)
{
    if (!ldm) return hb_fail(HB_ERR_INVALID, "hb_cg_run_ldm: null LD matrix handle");
    return cg_run(args, ldm, out, false);
}

extern "C" int hb_cg_run_sparse(const hb_cg_args *args, hb_ldm *ldm, hb_cg_out *out)
{
    if (!ldm) return hb_fail(HB_ERR_INVALID, "hb_cg_run_sparse: null LD matrix handle");
    return cg_run(args, ldm, out, true);
}
