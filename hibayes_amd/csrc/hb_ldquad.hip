// hb_ldquad.hip — the variance explained by windows of markers for the summary-level model, on the device: item (8) of the reference README's
// list, "phenotypic/genetic variance explained (PVE) by single or multiple SNPs", where there are no genotypes and the quantity is the quadratic
// form alpha_w' V_ww alpha_w on the LD matrix that ldmat() left with the library and SBayesD() / SBayesS() swept (R/sbayes.r:231-234 stops at the
// windows' WPPA). DESIGN.md §23. A unit of its own: it shares hb_wave.hpp (the wave and block sums) and the handle (hb_ldm.hpp) with the others;
// hb_ldqplan.hpp decides the list, the segments and the effects' table of a batch of at most 8 records.
//
//     k_ldq_cols_dense   columns of the dense device copy, 8 B per entry, coalesced    } one wave per listed column j. Lane l takes the column's
//     k_ldq_cols_csc     the column's run in the device CSC (rows sorted)              } entries l, l + 64, ... in that order, and for each entry
//                        (i, V) whose row has an effect in the batch and each record r adds (alpha_ir != 0 ? V alpha_ir : 0.0) to T[r] and, where
//                        row i lies in j's window, to t[r]; the wave's 64 by hb_wave.hpp's shuffle tree; lane 0 stores
//                        (alpha_jr != 0 ? alpha_jr t[r] : 0.0) and the same of T[r] at marker j. One body (ldq_cols), the loader is its argument.
//     k_ldq_windows      thread = (segment, record): the window's columns added in list order, which is marker order
//     k_ldq_total        workgroup = record: thread k adds markers k, k + 256, ... (a marker that is not listed holds 0.0), then the block sum
//     k_ldq_diag_*       V_jj from the same copy (0.0 where the sparse matrix stores none)
// A select, never a multiplication by an effect of 0.0: the sparse kinds keep NaN entries for monomorphic markers, and one reaches a result only
// where both effects are non-zero. No floating-point atomic, no clamp (a thresholded matrix is indefinite: a negative form is stored as computed).
// What a (window, record) value gets depends on the window's own effects in that record and the matrix: the other records of the batch, the other
// windows and the ids add 0.0 or nothing. The unit is compiled with -ffp-contract=off: products and sums round as written. No kernel uses scratch
// (hb_ldquad.res.txt; tests/test_ldpve_host.py).
#include "hb_internal.hpp"
#include "hb_wave.hpp"
#include "hb_ldm.hpp"
#include "hb_ldqplan.hpp"
#include <cmath>

namespace {

constexpr int RB = HB_LDQ_RB;

struct ld_dense {
    const double *V;
    int m;
    __device__ __forceinline__ int count(int) const { return m; }
    __device__ __forceinline__ void at(int j, int k, int &i, double &v) const { i = k, v = V[(size_t)j * (size_t)m + (size_t)k]; }
    __device__ __forceinline__ double diag(int j) const { return V[(size_t)j * (size_t)m + (size_t)j]; }
};

struct ld_csc {
    const int64_t *cp;
    const int32_t *ri;
    const double *va;
    __device__ __forceinline__ int count(int j) const { return (int)(cp[j + 1] - cp[j]); }
    __device__ __forceinline__ void at(int j, int k, int &i, double &v) const { i = ri[cp[j] + k], v = va[cp[j] + k]; }
    __device__ __forceinline__ double diag(int j) const
    {
        int64_t lo = cp[j], hi = cp[j + 1];
        while (lo < hi) { // the first entry with row >= j
            const int64_t mid = lo + (hi - lo) / 2;
            if (ri[mid] < j) lo = mid + 1;
            else hi = mid;
        }
        return lo < cp[j + 1] && ri[lo] == j ? va[lo] : 0.0;
    }
};

// idx: the list; aw: [m][RB] effects; win: [m] window id of a row with an effect in the batch, else 0; cw, cT: [m][RB], written at the listed markers
template <class LD>
__device__ __forceinline__ void ldq_cols(const LD L, int nnz, const int *__restrict__ idx, const double *__restrict__ aw,
                                         const uint32_t *__restrict__ win, double *__restrict__ cw, double *__restrict__ cT)
{
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= nnz) return; // (the whole wave)
    const int j = idx[e];
    const uint32_t wj = win[j];
    const int cnt = L.count(j);
    double t[RB], T[RB];
#pragma unroll
    for (int r = 0; r < RB; r++) t[r] = 0.0, T[r] = 0.0;
    for (int k = lane; k < cnt; k += 64) {
        int i;
        double v;
        L.at(j, k, i, v);
        const uint32_t wi = win[i];
        if (wi) {
            const bool in = wi == wj;
            const double *a = aw + (size_t)i * RB;
#pragma unroll
            for (int r = 0; r < RB; r++) {
                const double ar = a[r];
                const double term = ar != 0.0 ? v * ar : 0.0;
                T[r] += term;
                t[r] += in ? term : 0.0;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RB; r++) {
        t[r] = wave_sum(t[r]);
        T[r] = wave_sum(T[r]);
    }
    if (lane == 0) {
        const double *a = aw + (size_t)j * RB;
#pragma unroll
        for (int r = 0; r < RB; r++) {
            const double ar = a[r];
            cw[(size_t)j * RB + r] = ar != 0.0 ? ar * t[r] : 0.0;
            cT[(size_t)j * RB + r] = ar != 0.0 ? ar * T[r] : 0.0;
        }
    }
}

__global__ __launch_bounds__(256) void k_ldq_cols_dense(const double *__restrict__ V, int m, int nnz, const int *__restrict__ idx,
                                                        const double *__restrict__ aw, const uint32_t *__restrict__ win, double *__restrict__ cw,
                                                        double *__restrict__ cT)
{
    ldq_cols(ld_dense{V, m}, nnz, idx, aw, win, cw, cT);
}

__global__ __launch_bounds__(256) void k_ldq_cols_csc(const int64_t *__restrict__ cp, const int32_t *__restrict__ ri, const double *__restrict__ va,
                                                      int nnz, const int *__restrict__ idx, const double *__restrict__ aw,
                                                      const uint32_t *__restrict__ win, double *__restrict__ cw, double *__restrict__ cT)
{
    ldq_cols(ld_csc{cp, ri, va}, nnz, idx, aw, win, cw, cT);
}

// segs: {window, first, count} per segment; out: [window][RB]
__global__ __launch_bounds__(256) void k_ldq_windows(const double *__restrict__ cw, const int *__restrict__ idx, const int *__restrict__ segs, int nseg,
                                                     double *__restrict__ out)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nseg * RB) return;
    const int s = q / RB, r = q % RB;
    const int e_beg = segs[3 * s + 1], e_end = e_beg + segs[3 * s + 2];
    double sum = 0.0;
    for (int e = e_beg; e < e_end; e++) sum += cw[(size_t)idx[e] * RB + r];
    out[(size_t)segs[3 * s] * RB + r] = sum;
}

// out: [RB]; an order that depends on m alone
__global__ __launch_bounds__(256) void k_ldq_total(const double *__restrict__ cT, int m, double *__restrict__ out)
{
    __shared__ double red[4];
    const int r = blockIdx.x;
    double sum = 0.0;
    for (int j = threadIdx.x; j < m; j += 256) sum += cT[(size_t)j * RB + r];
    sum = block_sum(sum, red);
    if (threadIdx.x == 0) out[r] = sum;
}

template <class LD>
__device__ __forceinline__ void ldq_diag(const LD L, int m, double *__restrict__ out)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < m) out[j] = L.diag(j);
}

__global__ __launch_bounds__(256) void k_ldq_diag_dense(const double *__restrict__ V, int m, double *__restrict__ out) { ldq_diag(ld_dense{V, m}, m, out); }

__global__ __launch_bounds__(256) void k_ldq_diag_csc(const int64_t *__restrict__ cp, const int32_t *__restrict__ ri, const double *__restrict__ va, int m,
                                                      double *__restrict__ out)
{
    ldq_diag(ld_csc{cp, ri, va}, m, out);
}

} // namespace

extern "C" {

int hb_ldm_window_var(hb_ldm *l, const double *A, int64_t ldA, int32_t rows, int32_t R, const uint32_t *windindx, int32_t nw, double *var_out, int64_t ldv,
                      double *total_out)
{
    if (!l) return hb_fail(HB_ERR_INVALID, "hb_ldm_window_var: null handle");
    if (!var_out || !total_out || ldv < nw) return hb_fail(HB_ERR_INVALID, "hb_ldm_window_var: bad argument");
    if (rows != l->m) return hb_fail(HB_ERR_INVALID, "hb_ldm_window_var: the effects must have one row per marker of the matrix (" + std::to_string(l->m) + ")");
    const int m = l->m;
    const std::string refused = hb_ldq_check(A, ldA, m, R, windindx, nw);
    if (!refused.empty()) return hb_fail(HB_ERR_INVALID, "hb_ldm_window_var: " + refused);
    HB_HIP(hipSetDevice(l->device));
    // the loader follows the handle's kind alone, never the copies it happens to hold
    const bool dense = l->kind == HB_LDM_KIND_DENSE;
    const double *V = nullptr;
    hb_ldm_csc csc{};
    if (dense) HB_TRY(hb_ldm_device_dense(l, &V));
    else HB_TRY(hb_ldm_device_csc(l, &csc));
    const size_t seg_cap = (size_t)std::min(m, nw);
    hb_bufs bufs;
    int *didx = nullptr, *dsegs = nullptr;
    uint32_t *dwin = nullptr;
    double *daw = nullptr, *dcw = nullptr, *dcT = nullptr, *dout = nullptr;
    HB_TRY(bufs.get(&didx, (size_t)m));
    HB_TRY(bufs.get(&dsegs, 3 * seg_cap));
    HB_TRY(bufs.get(&dwin, (size_t)m));
    HB_TRY(bufs.get(&daw, (size_t)m * RB));
    HB_TRY(bufs.get(&dcw, (size_t)m * RB));
    HB_TRY(bufs.get(&dcT, (size_t)m * RB));
    HB_TRY(bufs.get(&dout, (size_t)(nw + 1) * RB));
    std::vector<int> hsegs;
    std::vector<double> hout((size_t)(nw + 1) * RB);
    for (int r0 = 0; r0 < R; r0 += RB) {
        const int nr = std::min(RB, R - r0);
        const hb_ldqplan p = hb_ldqplan_of(A + (size_t)r0 * ldA, ldA, m, nr, windindx, nw);
        if (!p.error.empty()) return hb_fail(HB_ERR_INVALID, "hb_ldm_window_var: " + p.error);
        const int nnz = (int)p.idx.size(), nseg = (int)p.segs.size();
        if (nnz) {
            hsegs.clear();
            for (const hb_ldqseg &s : p.segs) hsegs.insert(hsegs.end(), {s.window, s.first, s.count});
            HB_HIP(hipMemcpy(didx, p.idx.data(), sizeof(int) * nnz, hipMemcpyHostToDevice));
            HB_HIP(hipMemcpy(dsegs, hsegs.data(), sizeof(int) * hsegs.size(), hipMemcpyHostToDevice));
            HB_HIP(hipMemcpy(dwin, p.win.data(), sizeof(uint32_t) * m, hipMemcpyHostToDevice));
            HB_HIP(hipMemcpy(daw, p.aw.data(), sizeof(double) * (size_t)m * RB, hipMemcpyHostToDevice));
            HB_HIP(hipMemset(dcT, 0, sizeof(double) * (size_t)m * RB));         // (a marker that is not listed: 0.0 in the total's sum)
            HB_HIP(hipMemset(dout, 0, sizeof(double) * (size_t)(nw + 1) * RB)); // (a window that is never visited: 0.0 exactly)
            const dim3 grid((unsigned)((nnz + 3) / 4));
            if (dense) hipLaunchKernelGGL(k_ldq_cols_dense, grid, dim3(256), 0, 0, V, m, nnz, didx, daw, dwin, dcw, dcT);
            else hipLaunchKernelGGL(k_ldq_cols_csc, grid, dim3(256), 0, 0, csc.cp, csc.ri, csc.va, nnz, didx, daw, dwin, dcw, dcT);
            HB_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_ldq_windows, dim3((unsigned)((nseg * RB + 255) / 256)), dim3(256), 0, 0, dcw, didx, dsegs, nseg, dout);
            HB_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_ldq_total, dim3(RB), dim3(256), 0, 0, dcT, m, dout + (size_t)nw * RB);
            HB_HIP(hipGetLastError());
            HB_HIP(hipMemcpy(hout.data(), dout, sizeof(double) * hout.size(), hipMemcpyDeviceToHost));
        } else {
            std::fill(hout.begin(), hout.end(), 0.0);
        }
        for (int r = 0; r < nr; r++) {
            for (int w = 0; w < nw; w++) var_out[(size_t)(r0 + r) * ldv + w] = hout[(size_t)w * RB + r];
            total_out[r0 + r] = hout[(size_t)nw * RB + r];
        }
    }
    return HB_OK;
}

int hb_ldm_diagonal(hb_ldm *l, double *out)
{
    if (!l || !out) return hb_fail(HB_ERR_INVALID, "hb_ldm_diagonal: null argument");
    const int m = l->m;
    HB_HIP(hipSetDevice(l->device));
    hb_bufs bufs;
    double *d = nullptr;
    HB_TRY(bufs.get(&d, (size_t)m));
    const dim3 grid((unsigned)((m + 255) / 256));
    if (l->kind == HB_LDM_KIND_DENSE) {
        const double *V = nullptr;
        HB_TRY(hb_ldm_device_dense(l, &V));
        hipLaunchKernelGGL(k_ldq_diag_dense, grid, dim3(256), 0, 0, V, m, d);
    } else {
        hb_ldm_csc csc{};
        HB_TRY(hb_ldm_device_csc(l, &csc));
        hipLaunchKernelGGL(k_ldq_diag_csc, grid, dim3(256), 0, 0, csc.cp, csc.ri, csc.va, m, d);
    }
    HB_HIP(hipGetLastError());
    HB_HIP(hipMemcpy(out, d, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost));
    return HB_OK;
}

} // extern "C"
