// hb_ldmat.hip — the LD variance-covariance matrix of the resident genotypes: ldmat() of the reference (R/ldm.r:31-112) as
// tXXmat_Geno / tXXmat_Chr compute it (src/tXXmat.cpp:100-206, :504-626), without the four *_gwas variants.
//
// The work is the m x m integer contraction X'X over int8 columns — the staged tile loop of hb_mma.hpp (k_gram_tiled's) on arbitrary
// column pairs — followed per entry by the reference's own fp64 arithmetic, one correctly rounded operation at a time and in its order:
// the cross-products are exact integers, so every entry equals the reference's in every bit. Three things that arithmetic fixes:
//   * it is not symmetric in its two markers: `ind * m1 * m2` is (ind * m1) * m2 with m1 the mean of the marker of the SMALLER
//     index (the outer loop's j, :130-145), so each entry is computed with min(row, col) in the sum1 / m1 / p1 role;
//   * the dense paths write xx * xx / ind on the diagonal (:168, :582), the sparse paths send the diagonal through the
//     cross-product formula and the threshold like any other entry (:137-153, :543-560);
//   * the sparse test is `r * r * ind <= chisq` -> drop, so a NaN r (monomorphic marker) keeps its entry.
// The matrix is built a strip of columns at a time: all m rows x w columns into an fp64 staging strip (the strip bounds device
// memory and needs no mirrored writes), the strip goes to pinned host memory as it is (genome-wide dense) or compacted to
// row-sorted (row, value) lists per column (k_ld_compact: every other kind, the reference returns sp_mat there).
// This whole unit is compiled with floating-point contraction off (Makefile and the pragma below): hipcc fuses by default.
#include "hb_ldm.hpp"
#include "hb_mma.hpp"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <numeric>

#pragma clang fp contract(off)

namespace {
// ---- BigStat (src/tXXmat.cpp:43-77): mean = sum / ind, xx = sqrt(sum_k (x_k - mean)^2), the squares added in row order ----
// One lane per column (set-up work: m lanes x n dependent adds). X points at column col0; the column sums are k_stats' exact
// integers (hb_ctx::s1), which is what the reference's fp64 running sum of small integers holds too.
__global__ __launch_bounds__(64) void k_ld_stats(const int8_t *__restrict__ X, int64_t ld, int n, int col0, int ncols,
                                                 const double *__restrict__ sum, double *__restrict__ mean, double *__restrict__ xx)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= ncols) return;
    const int j = col0 + k;
    const double mu = sum[j] / (double)n;
    const int8_t *col = X + (int64_t)k * ld;
    double p1 = 0.0;
    for (int64_t r0 = 0; r0 < n; r0 += 16) { // (ld is a multiple of 256: the last 16 bytes are inside the column)
        const int4 v = *reinterpret_cast<const int4 *>(col + r0);
        const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (r0 + q * 4 + b < n) {
                    const double d = (double)(int)(int8_t)(w[q] >> (8 * b)) - mu;
                    p1 += d * d;
                }
    }
    mean[j] = mu;
    xx[j] = sqrt(p1);
}

struct ld_epi {
    const double *sum, *mean, *xx; // by marker
    const int32_t *chr;            // by marker, or nullptr: one block
    double ind, chisq;
};

// ---- one strip: rows = all markers, columns = positions [c0, c0 + w) of the column order perm[] ----
// hb_mma.hpp's staged loop (the one k_gram_tiled runs): a 256 x 256 tile per workgroup of 16 waves, 2 x 2 v_mfma_i32_32x32x32_i8 per
// wave. The strip's columns are the MFMA's A operand (accumulator registers) and the matrix' rows its B operand (lanes), so
// that a wave's stores run along a column of the column-major strip. Both operand sets go through perm[]; positions past the
// ragged end read the last valid column and are masked at the store. XA / XB: where genotype column 0 WOULD be (windows of a
// 2-bit resident matrix). Row tiles [rt0, rt0 + nrt) are this launch's. tchr (block mode): min / max chromosome id of every
// 256-tile of positions — a tile whose two ranges are disjoint holds zeros only and is left to the strip's memset.
template <bool SPARSE> // (a template, not a run-time switch: the arm not taken costs its fp64 division per element otherwise)
__global__ __launch_bounds__(1024) void k_ld_strip(const int8_t *__restrict__ XA, const int8_t *__restrict__ XB, int64_t ld, int m,
                                                   const int32_t *__restrict__ perm, int c0, int w, int rt0, int nrt,
                                                   const int32_t *__restrict__ tchr, ld_epi e, double *__restrict__ strip)
{
    __shared__ __attribute__((aligned(16))) char sa[MMA_T * MMA_CS], sb[MMA_T * MMA_CS];
    const int tj = rt0 + (int)(blockIdx.x % (unsigned)nrt), ti = (int)(blockIdx.x / (unsigned)nrt);
    if (tchr) { // (uniform per workgroup, before the first barrier)
        const int ct = c0 / MMA_T + ti;
        if (tchr[2 * tj + 1] < tchr[2 * ct] || tchr[2 * ct + 1] < tchr[2 * tj]) return;
    }
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wr = wave >> 2, wc = wave & 3;
    const int cend = c0 + w; // (<= m)
    const int8_t *ga = XA + (int64_t)perm[min(c0 + ti * MMA_T + mma_stage_col(tid), cend - 1)] * ld + mma_stage_part(tid) * 16;
    const int8_t *gb = XB + (int64_t)perm[min(tj * MMA_T + mma_stage_col(tid), m - 1)] * ld + mma_stage_part(tid) * 16;
    v16i acc[2][2];
    mma_i8_zero(acc);
    mma_i8_staged(acc, ga, gb, ld, sa, sb, tid);
    // ---- epilogue: src/tXXmat.cpp:145-152 / :168 / :177-179 per accumulator element, j = the smaller marker index ----
    // C/D layout: the lane carries the B operand's column (here: the matrix row), the register the A operand's (the strip column)
    int rowm[2];
    bool rok[2];
    double rs[2], rm[2], rx[2];
    int rc[2];
#pragma unroll
    for (int b = 0; b < 2; b++) {
        const int rp = tj * MMA_T + wc * 64 + mma_i8_col(b, lane);
        rok[b] = rp < m;
        rowm[b] = perm[min(rp, m - 1)];
        rs[b] = e.sum[rowm[b]];
        rm[b] = e.mean[rowm[b]];
        rx[b] = e.xx[rowm[b]];
        rc[b] = e.chr ? e.chr[rowm[b]] : 0;
    }
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int cp = c0 + ti * MMA_T + wr * 64 + mma_i8_row(a, r, lane);
            if (cp >= cend) continue;
            const int colm = perm[cp];
            const double cs = e.sum[colm], cm = e.mean[colm], cx = e.xx[colm];
            const int cc = e.chr ? e.chr[colm] : 0;
            double *out = strip + (size_t)(cp - c0) * (size_t)m;
#pragma unroll
            for (int b = 0; b < 2; b++) {
                if (!rok[b]) continue;
                const bool row_first = rowm[b] < colm;
                const double sj = row_first ? rs[b] : cs, mj = row_first ? rm[b] : cm, xj = row_first ? rx[b] : cx;
                const double si = row_first ? cs : rs[b], mi = row_first ? cm : rm[b], xi = row_first ? cx : rx[b];
                double p12 = (double)acc[a][b][r];
                p12 = p12 - (((sj * mi) + (si * mj)) - ((e.ind * mj) * mi));
                double val = p12 / e.ind;
                if (SPARSE) {
                    const double rr = p12 / (xj * xi);
                    if ((rr * rr) * e.ind <= e.chisq) val = 0.0;
                } else if (rowm[b] == colm) {
                    val = (xj * xj) / e.ind;
                }
                if (rc[b] != cc) val = 0.0;
                out[rowm[b]] = val;
            }
        }
}

// ---- strip -> per-column row-sorted (row, value) lists: one wave per strip column, ballot-prefix over the rows in order ----
// off == nullptr: count only (cnt[col]); otherwise column col's entries go to idx / val at off[col]. An entry is stored iff
// value != 0: an assigned 0 is not stored by arma::sp_mat either.
__global__ __launch_bounds__(256) void k_ld_compact(const double *__restrict__ strip, int m, int w, const int64_t *__restrict__ off,
                                                    int32_t *__restrict__ cnt, int32_t *__restrict__ idx, double *__restrict__ val)
{
    const int col = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (col >= w) return;
    const double *s = strip + (size_t)col * (size_t)m;
    const int64_t base = off ? off[col] : 0;
    int run = 0;
    for (int r0 = 0; r0 < m; r0 += 64) {
        const int r = r0 + lane;
        const double v = r < m ? s[r] : 0.0;
        const bool keep = r < m && v != 0.0;
        const unsigned long long mask = __ballot(keep);
        if (off && keep) {
            const int64_t p = base + run + __popcll(mask & ((1ull << lane) - 1ull));
            idx[p] = r;
            val[p] = v;
        }
        run += __popcll(mask);
    }
    if (!off && lane == 0) cnt[col] = run;
}

// strip column k -> column perm[c0 + k] of the dense device copy (rows are by marker already)
__global__ __launch_bounds__(256) void k_ld_scatter(const double *__restrict__ strip, int m, const int32_t *__restrict__ perm, int c0,
                                                    double *__restrict__ dense)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= m) return;
    dense[(size_t)perm[c0 + blockIdx.y] * (size_t)m + r] = strip[(size_t)blockIdx.y * (size_t)m + r];
}

// a chunk of compacted columns [j0, j0 + gridDim.x) -> the (zeroed) dense device copy; off is relative to the chunk
__global__ __launch_bounds__(256) void k_ld_densify(const int64_t *__restrict__ off, const int32_t *__restrict__ cnt,
                                                    const int32_t *__restrict__ idx, const double *__restrict__ val, int m, int j0,
                                                    double *__restrict__ dense)
{
    const int j = blockIdx.x;
    const int64_t o = off[j];
    for (int t = threadIdx.x; t < cnt[j]; t += 256) dense[(size_t)(j0 + j) * (size_t)m + idx[o + t]] = val[o + t];
}

int host_reserve(hb_ldm *l, int64_t need)
{
    if (need <= l->h_cap) return HB_OK;
    const int64_t cap = std::max<int64_t>(need, std::max<int64_t>(l->h_cap * 2, 1 << 16));
    int32_t *ni = nullptr;
    double *nv = nullptr;
    HB_TRY(l->mem.pin(&ni, (size_t)cap));
    if (l->mem.pin(&nv, (size_t)cap)) {
        l->mem.drop(&ni);
        return hb_fail(HB_ERR_HIP, "hb_ldm_build: out of pinned host memory");
    }
    if (l->h_used) {
        std::memcpy(ni, l->h_idx, sizeof(int32_t) * (size_t)l->h_used);
        std::memcpy(nv, l->h_val, sizeof(double) * (size_t)l->h_used);
    }
    l->mem.drop(&l->h_idx);
    l->mem.drop(&l->h_val);
    l->h_idx = ni;
    l->h_val = nv;
    l->h_cap = cap;
    return HB_OK;
}

int build(hb_ctx *c, const int32_t *chr, bool sparse, double chisq, int64_t strip_bytes, hb_ldm *l)
{
    const int m = c->m;
    const int64_t ld = c->ld;
    const bool use_chr = chr != nullptr;
    const auto t_all = hb_clk::now();
    hb_bufs D; // freed on every way out of the build
    // ---- where the int8 columns are: resident, or unpacked from the 2-bit layout (whole if small, else a window at a time) ----
    int64_t wincols = std::max<int64_t>(MMA_T, ((int64_t)1 << 30) / ld / MMA_T * MMA_T);
    if (const char *ev = getenv("HB_LDM_WINDOW_COLS")) wincols = std::max<int64_t>(MMA_T, (int64_t)atoi(ev) / MMA_T * MMA_T); // (tests: force the windowed path)
    const int8_t *Xfull = c->X;
    int8_t *winA = nullptr, *winB = nullptr;
    if (!Xfull && wincols >= m) {
        HB_TRY(D.get(&winA, (size_t)ld * m));
        HB_TRY(hbk_unpack2(c, 0, m, winA));
        Xfull = winA;
    }
    // ---- BigStat ----
    auto t0 = hb_clk::now();
    double *d_mean = nullptr, *d_xx = nullptr;
    HB_TRY(D.get(&d_mean, m));
    HB_TRY(D.get(&d_xx, m));
    if (Xfull) {
        hipLaunchKernelGGL(k_ld_stats, dim3((m + 63) / 64), dim3(64), 0, c->stream, Xfull, ld, c->n, 0, m, c->s1, d_mean, d_xx);
    } else {
        HB_TRY(D.get(&winB, (size_t)ld * wincols));
        for (int r0 = 0; r0 < m; r0 += (int)wincols) {
            const int nr = (int)std::min<int64_t>(wincols, m - r0);
            HB_TRY(hbk_unpack2(c, r0, nr, winB));
            hipLaunchKernelGGL(k_ld_stats, dim3((nr + 63) / 64), dim3(64), 0, c->stream, winB, ld, c->n, r0, nr, c->s1, d_mean, d_xx);
        }
    }
    HB_HIP(hipGetLastError());
    HB_HIP(hipStreamSynchronize(c->stream));
    l->t_stats = hb_since(t0);
    // ---- column order: by chromosome (stable: a chromosome's markers stay in marker order, so a column's entries, which all
    // lie in its own chromosome, come out row-sorted) where whole columns can be gathered; marker order otherwise ----
    std::vector<int32_t> perm(m);
    std::iota(perm.begin(), perm.end(), 0);
    if (use_chr && Xfull) std::stable_sort(perm.begin(), perm.end(), [&](int32_t x, int32_t y) { return chr[x] < chr[y]; });
    const int ntile = (m + MMA_T - 1) / MMA_T;
    int32_t *d_perm = nullptr, *d_chr = nullptr, *d_tchr = nullptr;
    HB_TRY(D.get(&d_perm, m));
    HB_HIP(hipMemcpy(d_perm, perm.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice));
    if (use_chr) {
        std::vector<int32_t> tc(2 * (size_t)ntile);
        for (int t = 0; t < ntile; t++) {
            int32_t lo = chr[perm[t * MMA_T]], hi = lo;
            for (int p = t * MMA_T; p < std::min(m, (t + 1) * MMA_T); p++) {
                lo = std::min(lo, chr[perm[p]]);
                hi = std::max(hi, chr[perm[p]]);
            }
            tc[2 * t] = lo;
            tc[2 * t + 1] = hi;
        }
        HB_TRY(D.get(&d_chr, m));
        HB_TRY(D.get(&d_tchr, 2 * (size_t)ntile));
        HB_HIP(hipMemcpy(d_chr, chr, sizeof(int32_t) * m, hipMemcpyHostToDevice));
        HB_HIP(hipMemcpy(d_tchr, tc.data(), sizeof(int32_t) * tc.size(), hipMemcpyHostToDevice));
    }
    // ---- strip geometry: strip_bytes of staging (fp64 strip; for the compacted kinds also its (row, value) lists) ----
    const bool compacted = l->kind != HB_LDM_KIND_DENSE;
    const int64_t budget = strip_bytes > 0 ? strip_bytes : ((int64_t)1 << 30);
    const int64_t percol = (int64_t)m * (compacted ? 20 : 8);
    const int m_up = ntile * MMA_T;
    const int w = (int)std::min<int64_t>(std::min(m_up, 32768), std::max<int64_t>(MMA_T, budget / percol / MMA_T * MMA_T)); // (k_ld_scatter: one grid row per strip column)
    const size_t scount = (size_t)m * (size_t)std::min(w, m);
    double *d_strip = nullptr, *d_val = nullptr;
    int32_t *d_idx = nullptr, *d_cnt = nullptr;
    int64_t *d_off = nullptr;
    HB_TRY(D.get(&d_strip, scount));
    if (compacted) {
        HB_TRY(D.get(&d_val, scount));
        HB_TRY(D.get(&d_idx, scount));
        HB_TRY(D.get(&d_cnt, w));
        HB_TRY(D.get(&d_off, w));
        l->col_off.assign(m, 0);
        l->col_cnt.assign(m, 0);
    } else {
        HB_TRY(l->mem.pin(&l->h_dense, (size_t)m * (size_t)m));
    }
    if (!Xfull && !winA) HB_TRY(D.get(&winA, (size_t)ld * (size_t)std::min(w, m)));
    // a dense device copy for the sampler is kept when it fits beside the context and the staging with room to spare
    {
        size_t fr = 0, tot = 0;
        const size_t need = sizeof(double) * (size_t)m * (size_t)m;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess && need <= fr / 2) (void)l->mem.try_get(&l->d_dense, (size_t)m * (size_t)m); // (refused: nullptr and no error, built on demand)
    }
    ld_epi e{c->s1, d_mean, d_xx, d_chr, (double)c->n, chisq};
    const auto kstrip = sparse ? k_ld_strip<true> : k_ld_strip<false>;
    std::vector<int32_t> cnt(w);
    std::vector<int64_t> off(w);
    for (int c0 = 0; c0 < m; c0 += w) {
        const int ws = std::min(w, m - c0), ntc = (ws + MMA_T - 1) / MMA_T;
        t0 = hb_clk::now();
        if (use_chr) HB_HIP(hipMemsetAsync(d_strip, 0, sizeof(double) * (size_t)m * ws, c->stream)); // (tiles across chromosomes are skipped)
        if (Xfull) {
            hipLaunchKernelGGL(kstrip, dim3((unsigned)(ntile * ntc)), dim3(1024), 0, c->stream, Xfull, Xfull, ld, m, d_perm, c0, ws, 0,
                               ntile, d_tchr, e, d_strip);
        } else { // perm is the identity here: position = marker
            HB_TRY(hbk_unpack2(c, c0, ws, winA));
            for (int r0 = 0; r0 < m; r0 += (int)wincols) {
                const int nr = (int)std::min<int64_t>(wincols, m - r0), nrt = (nr + MMA_T - 1) / MMA_T;
                HB_TRY(hbk_unpack2(c, r0, nr, winB));
                hipLaunchKernelGGL(kstrip, dim3((unsigned)(nrt * ntc)), dim3(1024), 0, c->stream, winA - (int64_t)c0 * ld,
                                   winB - (int64_t)r0 * ld, ld, m, d_perm, c0, ws, r0 / MMA_T, nrt, d_tchr, e, d_strip);
            }
        }
        HB_HIP(hipGetLastError());
        HB_HIP(hipStreamSynchronize(c->stream));
        l->t_strips += hb_since(t0);
        l->n_strips++;
        if (l->d_dense) {
            hipLaunchKernelGGL(k_ld_scatter, dim3((m + 255) / 256, ws), dim3(256), 0, c->stream, d_strip, m, d_perm, c0, l->d_dense);
            HB_HIP(hipGetLastError());
        }
        if (!compacted) {
            t0 = hb_clk::now();
            HB_HIP(hipMemcpyAsync(l->h_dense + (size_t)c0 * m, d_strip, sizeof(double) * (size_t)m * ws, hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
            l->t_xfer += hb_since(t0);
            continue;
        }
        t0 = hb_clk::now();
        hipLaunchKernelGGL(k_ld_compact, dim3((ws + 3) / 4), dim3(256), 0, c->stream, d_strip, m, ws, (const int64_t *)nullptr, d_cnt, d_idx, d_val);
        HB_HIP(hipGetLastError());
        HB_HIP(hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int32_t) * ws, hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        int64_t tot = 0;
        for (int k = 0; k < ws; k++) {
            off[k] = tot;
            tot += cnt[k];
        }
        HB_HIP(hipMemcpyAsync(d_off, off.data(), sizeof(int64_t) * ws, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_ld_compact, dim3((ws + 3) / 4), dim3(256), 0, c->stream, d_strip, m, ws, (const int64_t *)d_off, d_cnt, d_idx, d_val);
        HB_HIP(hipGetLastError());
        HB_HIP(hipStreamSynchronize(c->stream));
        l->t_compact += hb_since(t0);
        t0 = hb_clk::now();
        HB_TRY(host_reserve(l, l->h_used + tot));
        if (tot) {
            HB_HIP(hipMemcpyAsync(l->h_idx + l->h_used, d_idx, sizeof(int32_t) * (size_t)tot, hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipMemcpyAsync(l->h_val + l->h_used, d_val, sizeof(double) * (size_t)tot, hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
        }
        for (int k = 0; k < ws; k++) {
            l->col_off[perm[c0 + k]] = l->h_used + off[k];
            l->col_cnt[perm[c0 + k]] = cnt[k];
        }
        l->h_used += tot;
        l->t_xfer += hb_since(t0);
    }
    HB_HIP(hipStreamSynchronize(c->stream));
    // ---- the diagonal, for SBayesD()'s first lines ----
    l->diag.assign(m, 0.0);
    if (!compacted) {
        for (int j = 0; j < m; j++) l->diag[j] = l->h_dense[(size_t)j * m + j];
        l->nnz = (int64_t)m * m;
    } else {
        for (int j = 0; j < m; j++) {
            const int32_t *ib = l->h_idx + l->col_off[j], *ie = ib + l->col_cnt[j];
            const int32_t *it = std::lower_bound(ib, ie, (int32_t)j);
            if (it != ie && *it == j) l->diag[j] = l->h_val[l->col_off[j] + (it - ib)];
        }
        l->nnz = l->h_used;
    }
    l->seconds = hb_since(t_all);
    return HB_OK;
}
} // namespace

int hb_ldm_device_dense(hb_ldm *l, const double **out)
{
    HB_HIP(hipSetDevice(l->device));
    if (!l->d_dense) {
        const int m = l->m;
        double *d = nullptr;
        hb_bufs D;
        HB_TRY(D.get(&d, (size_t)m * (size_t)m)); // (the handle's below, once the copy is complete)
        if (l->kind == HB_LDM_KIND_DENSE) {
            HB_HIP(hipMemcpy(d, l->h_dense, sizeof(double) * (size_t)m * (size_t)m, hipMemcpyHostToDevice));
        } else {
            HB_HIP(hipMemset(d, 0, sizeof(double) * (size_t)m * (size_t)m));
            // the compacted columns in chunks of at most 2^26 entries
            int64_t *d_off = nullptr;
            int32_t *d_cnt = nullptr, *d_idx = nullptr;
            double *d_val = nullptr;
            const int64_t chunk = (int64_t)1 << 26;
            int rc;
            if ((rc = D.get(&d_off, m)) || (rc = D.get(&d_cnt, m)) || (rc = D.get(&d_idx, (size_t)std::min<int64_t>(chunk + m, std::max<int64_t>(l->nnz, 1)))) ||
                (rc = D.get(&d_val, (size_t)std::min<int64_t>(chunk + m, std::max<int64_t>(l->nnz, 1)))))
                return rc;
            std::vector<int64_t> off;
            std::vector<int32_t> idx;
            std::vector<double> val;
            for (int j0 = 0; j0 < m;) {
                off.clear();
                idx.clear();
                val.clear();
                int j1 = j0;
                while (j1 < m && (j1 == j0 || (int64_t)idx.size() + l->col_cnt[j1] <= chunk)) {
                    off.push_back((int64_t)idx.size());
                    idx.insert(idx.end(), l->h_idx + l->col_off[j1], l->h_idx + l->col_off[j1] + l->col_cnt[j1]);
                    val.insert(val.end(), l->h_val + l->col_off[j1], l->h_val + l->col_off[j1] + l->col_cnt[j1]);
                    j1++;
                }
                HB_HIP(hipMemcpy(d_off, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice));
                HB_HIP(hipMemcpy(d_cnt, l->col_cnt.data() + j0, sizeof(int32_t) * (size_t)(j1 - j0), hipMemcpyHostToDevice));
                if (!idx.empty()) {
                    HB_HIP(hipMemcpy(d_idx, idx.data(), sizeof(int32_t) * idx.size(), hipMemcpyHostToDevice));
                    HB_HIP(hipMemcpy(d_val, val.data(), sizeof(double) * val.size(), hipMemcpyHostToDevice));
                }
                hipLaunchKernelGGL(k_ld_densify, dim3((unsigned)(j1 - j0)), dim3(256), 0, 0, d_off, d_cnt, d_idx, d_val, m, j0, d);
                HB_HIP(hipGetLastError());
                HB_HIP(hipDeviceSynchronize());
                j0 = j1;
            }
        }
        D.give(l->mem, d);
        l->d_dense = d;
    }
    *out = l->d_dense;
    return HB_OK;
}

int hb_ldm_device_csc(hb_ldm *l, hb_ldm_csc *out)
{
    HB_HIP(hipSetDevice(l->device));
    if (!l->d_cp) {
        const int m = l->m;
        const bool dense = l->kind == HB_LDM_KIND_DENSE;
        std::vector<int64_t> cp(m + 1, 0), run(m, 0);
        std::vector<int32_t> cnt(m, 0), runn(m, 0);
        for (int j = 0; j < m; j++) {
            int32_t c = 0;
            if (dense) {
                const double *col = l->h_dense + (size_t)j * m;
                for (int r = 0; r < m; r++) c += col[r] != 0.0;
            } else {
                c = l->col_cnt[j];
            }
            // varediff counts what the matrix STORES (src/SBayesS.cpp:131-141): the genome-wide dense kind stores all m entries of a
            // column (hb_ldm_stats.nnz = m * m), its exact zeros are left out of the CSC only because walking them changes nothing
            cnt[j] = dense ? m : c;
            cp[j + 1] = cp[j] + c;
        }
        const int64_t nnz = cp[m];
        std::vector<int32_t> ri((size_t)std::max<int64_t>(nnz, 1));
        std::vector<double> va((size_t)std::max<int64_t>(nnz, 1));
        for (int j = 0; j < m; j++) {
            int64_t p = cp[j];
            if (dense) {
                const double *col = l->h_dense + (size_t)j * m;
                for (int r = 0; r < m; r++)
                    if (col[r] != 0.0) {
                        ri[p] = r;
                        va[p++] = col[r];
                    }
            } else if (cnt[j]) {
                std::memcpy(ri.data() + p, l->h_idx + l->col_off[j], sizeof(int32_t) * (size_t)l->col_cnt[j]);
                std::memcpy(va.data() + p, l->h_val + l->col_off[j], sizeof(double) * (size_t)l->col_cnt[j]);
            }
        }
        // per marker: its column's entries inside the rows of its own group; per group: the rows its columns touch
        const int ng = (m + HB_LDM_GS - 1) / HB_LDM_GS;
        l->grp_lo.assign(ng, 0);
        l->grp_hi.assign(ng, 0);
        for (int g = 0; g < ng; g++) {
            const int g0 = g * HB_LDM_GS, g1 = std::min(m, g0 + HB_LDM_GS);
            int32_t lo = m, hi = 0;
            for (int j = g0; j < g1; j++) {
                const int32_t *b = ri.data() + cp[j], *e = ri.data() + cp[j + 1];
                const int32_t *a = std::lower_bound(b, e, (int32_t)g0), *z = std::lower_bound(a, e, (int32_t)g1);
                run[j] = cp[j] + (a - b);
                runn[j] = (int32_t)(z - a);
                if (b != e) {
                    lo = std::min(lo, *b);
                    hi = std::max(hi, *(e - 1) + 1);
                }
            }
            if (lo < hi) {
                l->grp_lo[g] = lo;
                l->grp_hi[g] = hi;
            }
        }
        hb_bufs D;
        int64_t *d_cp = nullptr, *d_run = nullptr;
        int32_t *d_ri = nullptr, *d_cnt = nullptr, *d_runn = nullptr;
        double *d_va = nullptr;
        int rc;
        if ((rc = D.get(&d_cp, m + 1)) || (rc = D.get(&d_run, m)) || (rc = D.get(&d_ri, ri.size())) || (rc = D.get(&d_cnt, m)) ||
            (rc = D.get(&d_runn, m)) || (rc = D.get(&d_va, va.size())))
            return rc;
        HB_HIP(hipMemcpy(d_cp, cp.data(), sizeof(int64_t) * (m + 1), hipMemcpyHostToDevice));
        HB_HIP(hipMemcpy(d_run, run.data(), sizeof(int64_t) * m, hipMemcpyHostToDevice));
        HB_HIP(hipMemcpy(d_cnt, cnt.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice));
        HB_HIP(hipMemcpy(d_runn, runn.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice));
        HB_HIP(hipMemcpy(d_ri, ri.data(), sizeof(int32_t) * ri.size(), hipMemcpyHostToDevice));
        HB_HIP(hipMemcpy(d_va, va.data(), sizeof(double) * va.size(), hipMemcpyHostToDevice));
        for (void *q : {(void *)d_cp, (void *)d_run, (void *)d_ri, (void *)d_cnt, (void *)d_runn, (void *)d_va}) D.give(l->mem, q); // the handle's from here
        l->d_run = d_run;
        l->d_ri = d_ri;
        l->d_cnt = d_cnt;
        l->d_runn = d_runn;
        l->d_va = d_va;
        l->csc_nnz = nnz;
        l->d_cp = d_cp;
    }
    *out = hb_ldm_csc{l->csc_nnz, l->d_cp, l->d_run, l->d_ri, l->d_cnt, l->d_runn, l->d_va, l->grp_lo.data(), l->grp_hi.data()};
    return HB_OK;
}

extern "C" {

void hb_ldm_destroy(hb_ldm *l)
{
    if (!l) return;
    if (!l->mem.dev.empty() || !l->mem.pinned.empty()) (void)hipSetDevice(l->device);
    delete l;
}

int hb_ldm_build(hb_ctx *c, const int32_t *chr, int32_t has_chisq, double chisq, int64_t strip_bytes, hb_ldm **out)
{
    if (!c || !out) return hb_fail(HB_ERR_INVALID, "hb_ldm_build: null argument");
    *out = nullptr;
    if (c->layout == 64)
        return hb_fail(HB_ERR_UNSUPPORTED, "hb_ldm_build: the context holds the fp64 resident layout (real-valued genotypes); the LD matrix is built from integer genotypes");
    if (!hb_ctx_has_genotypes(c) || (!c->X && !c->X2)) return hb_fail(HB_ERR_INVALID, "hb_ldm_build: no genotypes on the device");
    if (strip_bytes < 0) return hb_fail(HB_ERR_INVALID, "hb_ldm_build: strip_bytes must be >= 0");
    if (c->row_reduce) return hb_fail(HB_ERR_UNSUPPORTED, "hb_ldm_build: a row-sharded context holds a block of individuals only");
    HB_HIP(hipSetDevice(c->device));
    if (!c->stats_ready) {
        int rc = hbk_stats(c);
        if (rc) return rc;
    }
    const double amax = std::max(std::abs((double)c->xmin), std::abs((double)c->xmax));
    if (amax * amax * (double)c->n >= 2147483647.0)
        return hb_fail(HB_ERR_UNSUPPORTED, "genotype codes too large for the exact int32 Gram matrix at this n");
    // the mode, as the reference picks it: genome-wide (src/tXXmat.cpp:117-120) sparse iff chisq > 0; per chromosome (:520-523)
    // sparse iff chisq is given at all
    const bool sparse = chr ? has_chisq != 0 : (has_chisq != 0 && chisq > 0);
    hb_ldm *l = new hb_ldm();
    l->device = c->device;
    l->m = c->m;
    l->kind = chr ? (sparse ? HB_LDM_KIND_BLOCK_SPARSE : HB_LDM_KIND_BLOCK_DENSE) : (sparse ? HB_LDM_KIND_SPARSE : HB_LDM_KIND_DENSE);
    const int rc = build(c, chr, sparse, chisq, strip_bytes, l);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        hb_ldm_destroy(l);
        return rc;
    }
    *out = l;
    return HB_OK;
}

int hb_ldm_from_csc(int32_t m, const int64_t *indptr, const int32_t *indices, const double *data, int32_t device, hb_ldm **out)
{
    if (!out) return hb_fail(HB_ERR_INVALID, "hb_ldm_from_csc: null argument");
    *out = nullptr;
    if (m < 1 || !indptr) return hb_fail(HB_ERR_INVALID, "hb_ldm_from_csc: null argument");
    if (indptr[0] != 0) return hb_fail(HB_ERR_INVALID, "hb_ldm_from_csc: indptr must start at 0");
    for (int j = 0; j < m; j++)
        if (indptr[j + 1] < indptr[j] || indptr[j + 1] - indptr[j] > m) return hb_fail(HB_ERR_INVALID, "hb_ldm_from_csc: indptr must not decrease");
    const int64_t nnz = indptr[m];
    if (nnz && (!indices || !data)) return hb_fail(HB_ERR_INVALID, "hb_ldm_from_csc: null argument");
    for (int j = 0; j < m; j++)
        for (int64_t p = indptr[j]; p < indptr[j + 1]; p++) {
            if (indices[p] < 0 || indices[p] >= m) return hb_fail(HB_ERR_INVALID, "hb_ldm_from_csc: row index out of range");
            if (p > indptr[j] && indices[p] <= indices[p - 1])
                return hb_fail(HB_ERR_INVALID, "hb_ldm_from_csc: row indices must be sorted and unique inside a column");
        }
    for (int j = 0; j < m; j++) // entry (r, j) needs its mirror (j, r) with the same bits
        for (int64_t p = indptr[j]; p < indptr[j + 1]; p++) {
            const int r = indices[p];
            if (r == j) continue;
            const int32_t *b = indices + indptr[r], *e = indices + indptr[r + 1];
            const int32_t *it = std::lower_bound(b, e, (int32_t)j);
            if (it == e || *it != j || std::memcmp(data + (it - indices), data + p, sizeof(double)) != 0)
                return hb_fail(HB_ERR_INVALID, "hb_ldm_from_csc: the matrix must equal its transpose, in pattern and in value bits");
        }
    if (hb_device_count() <= 0) return hb_fail(HB_ERR_NO_DEVICE, "no HIP device available: the hibayes GPU engine has no CPU fallback");
    if (device < 0 || device >= hb_device_count()) return hb_fail(HB_ERR_INVALID, "hb_ldm_from_csc: no such device");
    HB_HIP(hipSetDevice(device));
    hb_ldm *l = new hb_ldm();
    l->device = device;
    l->m = m;
    l->kind = HB_LDM_KIND_SPARSE;
    const int rc = host_reserve(l, std::max<int64_t>(nnz, 1));
    if (rc) {
        hb_ldm_destroy(l);
        return rc;
    }
    if (nnz) {
        std::memcpy(l->h_idx, indices, sizeof(int32_t) * (size_t)nnz);
        std::memcpy(l->h_val, data, sizeof(double) * (size_t)nnz);
    }
    l->h_used = l->nnz = nnz;
    l->col_off.assign(indptr, indptr + m);
    l->col_cnt.resize(m);
    l->diag.assign(m, 0.0);
    for (int j = 0; j < m; j++) {
        l->col_cnt[j] = (int32_t)(indptr[j + 1] - indptr[j]);
        const int32_t *b = indices + indptr[j], *e = indices + indptr[j + 1];
        const int32_t *it = std::lower_bound(b, e, (int32_t)j);
        if (it != e && *it == j) l->diag[j] = data[it - indices];
    }
    *out = l;
    return HB_OK;
}

int hb_ldm_info(const hb_ldm *l, hb_ldm_stats *s)
{
    if (!l || !s) return hb_fail(HB_ERR_INVALID, "hb_ldm_info: null argument");
    s->m = l->m;
    s->kind = l->kind;
    s->on_device = l->d_dense != nullptr;
    s->n_strips = l->n_strips;
    s->nnz = l->nnz;
    s->seconds = l->seconds;
    s->stats_seconds = l->t_stats;
    s->strip_seconds = l->t_strips;
    s->compact_seconds = l->t_compact;
    s->transfer_seconds = l->t_xfer;
    return HB_OK;
}

int hb_ldm_download_dense(hb_ldm *l, double *out, int64_t ldo)
{
    if (!l || !out || ldo < l->m) return hb_fail(HB_ERR_INVALID, "hb_ldm_download_dense: bad argument");
    const int m = l->m;
    for (int j = 0; j < m; j++) {
        double *o = out + (size_t)j * (size_t)ldo;
        if (l->kind == HB_LDM_KIND_DENSE) {
            std::memcpy(o, l->h_dense + (size_t)j * m, sizeof(double) * m);
        } else {
            std::memset(o, 0, sizeof(double) * m);
            for (int32_t t = 0; t < l->col_cnt[j]; t++) o[l->h_idx[l->col_off[j] + t]] = l->h_val[l->col_off[j] + t];
        }
    }
    return HB_OK;
}

int hb_ldm_download_csc(hb_ldm *l, int64_t *indptr, int32_t *indices, double *data)
{
    if (!l || !indptr || (l->nnz && (!indices || !data))) return hb_fail(HB_ERR_INVALID, "hb_ldm_download_csc: null argument");
    if (l->kind == HB_LDM_KIND_DENSE) return hb_fail(HB_ERR_INVALID, "hb_ldm_download_csc: the handle holds the genome-wide dense matrix (hb_ldm_download_dense)");
    int64_t p = 0;
    for (int j = 0; j < l->m; j++) {
        indptr[j] = p;
        if (l->col_cnt[j]) {
            std::memcpy(indices + p, l->h_idx + l->col_off[j], sizeof(int32_t) * (size_t)l->col_cnt[j]);
            std::memcpy(data + p, l->h_val + l->col_off[j], sizeof(double) * (size_t)l->col_cnt[j]);
        }
        p += l->col_cnt[j];
    }
    indptr[l->m] = p;
    return HB_OK;
}

} // extern "C"
