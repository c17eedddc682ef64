// hb_pve.hip — the variance explained by windows of markers, on the device: item (8) of the reference README's list of what hibayes estimates,
// "phenotypic/genetic variance explained (PVE) by single or multiple SNPs". The reference leaves it to the user's R session, after the GEBV
// step of R/bayes.r:303-308 (MCMCsamples$g = M %*% MCMCsamples$alpha): apply(geno, 2, var) * alpha^2 / var(pheno), which is right for one marker
// and wrong for a window of markers in LD, where the quantity is var(X_w alpha_w). DESIGN.md §21. A unit of its own: it shares hb_wave.hpp (the
// wave sum, hb_ld4) with the others and nothing else; hb_pveplan.hpp decides the list, the segments, the shifts and the grid of a batch.
//
//     k_window_var       int8 columns, or 2-bit ones through hb_ld4      } thread = 4 rows x 8 records, workgroup = 1024 rows x a chunk of segments.
//     k_window_var_real  fp64 columns                                    } Per segment: g[row][r] by one fma per list entry in list order (k_xmat's
//                        chain), then t = g - c[w][r] for the rows < n, sum t and sum t^2 (the squares by fma) over the thread's rows in row order,
//                        the wave's 64 by hb_wave.hpp's shuffle tree, the four waves in wave order through LDS, and one (S1, S2) pair per record
//                        stored at [segment][row block]. One barrier per segment (the LDS slots alternate).
//     k_window_var_fin   thread = (segment, record): the row blocks' pairs added in row-block order, (S2 - S1^2 / n) / (n - 1) stored — R's var();
//                        a rounding that takes it below zero is stored as 0.0
// The total var(X alpha) of each record is one more segment over the whole list with a chunk of its own, in the same launch. (The other way, every
// thread keeping the running sum of its finished g, needs every workgroup to walk every segment: it rules the chunks out, and with them the grid
// that fills the chip; the extra segment costs at most what the windows cost and is one more column of workgroups beside theirs.)
// No floating-point atomic, no wait for another workgroup. What a (window, record) pair gets depends on its own list entries, on n and on nothing
// else: not on the other records of the batch (their entries add x * 0.0), not on the other windows, not on the chunks. None uses scratch
// (hb_pve.res.txt; tests/test_pve_host.py).
#include "hb_internal.hpp"
#include "hb_wave.hpp"
#include "hb_ldm.hpp"
#include "hb_pveplan.hpp"
#include <cmath>
#include <cstring>

namespace {

constexpr int RB = HB_PVE_RB;
static_assert(HB_PVE_ROWS == 256 * 4, "a workgroup of 256 threads x 4 rows");

struct ld_i8 {
    const int8_t *X;
    int64_t ld;
    const uint32_t *X2;
    int64_t ld2w;
    typedef int word;
    __device__ __forceinline__ word load(int col, int64_t row0) const { return hb_ld4(X, ld, X2, ld2w, col, row0); }
    __device__ __forceinline__ static double at(word w, int a) { return (double)(int8_t)(w >> (8 * a)); }
};

struct ld_real {
    const double *X;
    int64_t ld;
    struct word { d2 lo, hi; };
    __device__ __forceinline__ word load(int col, int64_t row0) const
    {
        const double *q = X + (int64_t)col * ld + row0;
        return word{*reinterpret_cast<const d2 *>(q), *reinterpret_cast<const d2 *>(q + 2)};
    }
    __device__ __forceinline__ static double at(const word &w, int a) { return a == 0 ? w.lo.x : a == 1 ? w.lo.y : a == 2 ? w.hi.x : w.hi.y; }
};

// segs: {window, first, count} per segment; chunks: {first segment, count}; part: [segment - seg_base][row block][2 RB] = S1[0 .. RB), S2[0 .. RB)
template <class LD>
__device__ __forceinline__ void window_var_body(const LD L, int n, int64_t ld, const int *__restrict__ idx, const double *__restrict__ val,
                                                const int *__restrict__ segs, const double *__restrict__ shift, const int *__restrict__ chunks,
                                                int chunk_base, int seg_base, double *__restrict__ part)
{
    __shared__ double red[2][4][2 * RB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rb = blockIdx.x, nrb = gridDim.x;
    const int64_t row0 = ((int64_t)rb * 256 + tid) * 4;
    const int64_t rowl = row0 < ld - 4 ? row0 : ld - 4; // (the last row block of a short matrix: its threads past ld load the last rows and drop them)
    const int *ch = chunks + 2 * (chunk_base + blockIdx.y);
    const int sbeg = ch[0], send = ch[0] + ch[1];
    int buf = 0;
    for (int s = sbeg; s < send; s++, buf ^= 1) {
        const int e_beg = segs[3 * s + 1], e_end = e_beg + segs[3 * s + 2];
        double acc[4][RB];
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int r = 0; r < RB; r++) acc[a][r] = 0.0;
        for (int e0 = e_beg; e0 < e_end; e0 += 4) {
            typename LD::word w[4];
#pragma unroll
            for (int k = 0; k < 4; k++) w[k] = L.load(idx[min(e0 + k, e_end - 1)], rowl);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (e0 + k < e_end) { // uniform
                    const double *v = val + (size_t)(e0 + k) * RB;
#pragma unroll
                    for (int a = 0; a < 4; a++) {
                        const double x = LD::at(w[k], a);
#pragma unroll
                        for (int r = 0; r < RB; r++) acc[a][r] = fma(x, v[r], acc[a][r]);
                    }
                }
            }
        }
        const double *c = shift + (size_t)s * RB;
        double s1[RB], s2[RB];
#pragma unroll
        for (int r = 0; r < RB; r++) {
            s1[r] = 0.0, s2[r] = 0.0;
            const double cr = c[r];
#pragma unroll
            for (int a = 0; a < 4; a++) {
                const double t = row0 + a < n ? acc[a][r] - cr : 0.0; // (padding rows contribute nothing)
                s1[r] += t;
                s2[r] = fma(t, t, s2[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < RB; r++) {
            s1[r] = wave_sum(s1[r]);
            s2[r] = wave_sum(s2[r]);
        }
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < RB; r++) {
                red[buf][wave][r] = s1[r];
                red[buf][wave][RB + r] = s2[r];
            }
        }
        __syncthreads();
        // (the slot written two segments on is this one again: a wave gets there only through the next barrier, which wave 0 passes after these reads)
        if (tid < 2 * RB) part[((size_t)(s - seg_base) * nrb + rb) * (2 * RB) + tid] = ((red[buf][0][tid] + red[buf][1][tid]) + red[buf][2][tid]) + red[buf][3][tid];
    }
}

__global__ __launch_bounds__(256) void k_window_var(const int8_t *__restrict__ X, int64_t ld, const uint32_t *__restrict__ X2, int64_t ld2w, int n,
                                                    const int *__restrict__ idx, const double *__restrict__ val, const int *__restrict__ segs,
                                                    const double *__restrict__ shift, const int *__restrict__ chunks, int chunk_base, int seg_base,
                                                    double *__restrict__ part)
{
    window_var_body(ld_i8{X, ld, X2, ld2w}, n, ld, idx, val, segs, shift, chunks, chunk_base, seg_base, part);
}

__global__ __launch_bounds__(256) void k_window_var_real(const double *__restrict__ X, int64_t ld, int n, const int *__restrict__ idx,
                                                         const double *__restrict__ val, const int *__restrict__ segs, const double *__restrict__ shift,
                                                         const int *__restrict__ chunks, int chunk_base, int seg_base, double *__restrict__ part)
{
    window_var_body(ld_real{X, ld}, n, ld, idx, val, segs, shift, chunks, chunk_base, seg_base, part);
}

// out: [window][RB], the total's segment names window nw
__global__ __launch_bounds__(256) void k_window_var_fin(const double *__restrict__ part, const int *__restrict__ segs, int seg_base, int nseg, int nrb,
                                                        int n, double *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nseg * RB) return;
    const int sl = i / RB, r = i % RB;
    const double *q = part + (size_t)sl * nrb * (2 * RB);
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < nrb; b++) {
        s1 += q[(size_t)b * (2 * RB) + r];
        s2 += q[(size_t)b * (2 * RB) + RB + r];
    }
    const double ss = s2 - s1 * s1 / (double)n;
    out[(size_t)segs[3 * (seg_base + sl)] * RB + r] = ss > 0.0 ? ss / (double)(n - 1) : 0.0;
}

constexpr size_t PART_CAP_BYTES = (size_t)128 << 20; // the partial pairs of one launch, unless a single chunk needs more

} // namespace

extern "C" {

int hb_pve_plan(const double *A, int64_t ldA, int32_t m, int32_t nr, const uint32_t *windindx, int32_t nw, const double *s1, int32_t n, int64_t ld,
                int32_t num_cus, int32_t *counts, int32_t *idx, double *val, int32_t *segs, double *shift, double *total_shift, int32_t *chunks)
{
    if (!counts || !idx || !val || !segs || !shift || !total_shift || !chunks) return hb_fail(HB_ERR_INVALID, "hb_pve_plan: null argument");
    const hb_pveplan p = hb_pveplan_of(A, ldA, m, nr, windindx, nw, s1, n, ld, num_cus);
    if (!p.error.empty()) return hb_fail(HB_ERR_INVALID, "hb_pve_plan: " + p.error);
    counts[0] = (int32_t)p.idx.size(), counts[1] = (int32_t)p.segs.size(), counts[2] = (int32_t)p.chunks.size(), counts[3] = p.row_blocks;
    std::copy(p.idx.begin(), p.idx.end(), idx);
    std::copy(p.val.begin(), p.val.end(), val);
    std::copy(p.shift.begin(), p.shift.end(), shift);
    std::copy(p.total_shift, p.total_shift + RB, total_shift);
    for (size_t s = 0; s < p.segs.size(); s++) segs[3 * s] = p.segs[s].window, segs[3 * s + 1] = p.segs[s].first, segs[3 * s + 2] = p.segs[s].count;
    for (size_t k = 0; k < p.chunks.size(); k++) chunks[2 * k] = p.chunks[k].first, chunks[2 * k + 1] = p.chunks[k].count;
    return HB_OK;
}

int hb_ctx_window_var(hb_ctx *c, const double *A, int64_t ldA, int32_t R, const uint32_t *windindx, int32_t nw, double *var_out, int64_t ldv,
                      double *total_out)
{
    if (!c) return hb_fail(HB_ERR_INVALID, "hb_ctx_window_var: null context");
    if (!A || !windindx || !var_out || !total_out || R < 0 || nw < 1 || ldA < c->m || ldv < nw) return hb_fail(HB_ERR_INVALID, "hb_ctx_window_var: bad argument");
    if (c->row_reduce)
        return hb_fail(HB_ERR_UNSUPPORTED, "hb_ctx_window_var: a row-sharded context holds a block of individuals only (a window's breeding values would have to be summed over the shards)");
    if (!hb_ctx_has_genotypes(c) || (!c->X && !c->X2 && !c->Xd)) return hb_fail(HB_ERR_INVALID, "hb_ctx_window_var: no genotypes on the device");
    if (c->n < 2) return hb_fail(HB_ERR_INVALID, "hb_ctx_window_var: a variance needs n >= 2 individuals");
    HB_HIP(hipSetDevice(c->device));
    if (!c->stats_ready) { // (2-bit only: the column sums were computed before the int8 copy was dropped and stay valid)
        if (c->layout != 64 && !c->X) return hb_fail(HB_ERR_INVALID, "hb_ctx_window_var: the context holds its genotypes in the 2-bit layout only and has no column sums");
        HB_TRY(hbk_stats(c));
    }
    if (R == 0) return HB_OK;
    const int m = c->m, n = c->n;
    std::vector<double> s1((size_t)m);
    HB_HIP(hipMemcpy(s1.data(), c->s1, sizeof(double) * m, hipMemcpyDeviceToHost));
    const int nrb = (n + HB_PVE_ROWS - 1) / HB_PVE_ROWS;
    const size_t seg_cap = (size_t)std::min(m, nw) + 1; // + the total's
    hb_bufs bufs;
    int *didx = nullptr, *dsegs = nullptr, *dchunks = nullptr;
    double *dval = nullptr, *dshift = nullptr, *dpart = nullptr, *dout = nullptr;
    HB_TRY(bufs.get(&didx, (size_t)m));
    HB_TRY(bufs.get(&dval, (size_t)m * RB));
    HB_TRY(bufs.get(&dsegs, 3 * seg_cap));
    HB_TRY(bufs.get(&dshift, RB * seg_cap));
    HB_TRY(bufs.get(&dchunks, 2 * seg_cap));
    HB_TRY(bufs.get(&dout, (size_t)(nw + 1) * RB));
    size_t part_segs = 0; // segments dpart holds
    std::vector<int> hsegs, hchunks;
    std::vector<double> hshift, hout((size_t)(nw + 1) * RB);
    for (int r0 = 0; r0 < R; r0 += RB) {
        const int nr = std::min(RB, R - r0);
        const hb_pveplan p = hb_pveplan_of(A + (size_t)r0 * ldA, ldA, m, nr, windindx, nw, s1.data(), n, c->ld, c->num_cus);
        if (!p.error.empty()) return hb_fail(HB_ERR_INVALID, "hb_ctx_window_var: " + p.error);
        const int nnz = (int)p.idx.size(), nseg = (int)p.segs.size(), nch = (int)p.chunks.size();
        if (nnz) {
            // the windows' segments and chunks, then the total's: one segment over the whole list, a chunk of its own
            hsegs.clear(), hchunks.clear();
            for (const hb_pveseg &s : p.segs) hsegs.insert(hsegs.end(), {s.window, s.first, s.count});
            hsegs.insert(hsegs.end(), {nw, 0, nnz});
            for (const hb_pvechunk &k : p.chunks) hchunks.insert(hchunks.end(), {k.first, k.count});
            hchunks.insert(hchunks.end(), {nseg, 1});
            hshift = p.shift;
            hshift.insert(hshift.end(), p.total_shift, p.total_shift + RB);
            HB_HIP(hipMemcpyAsync(didx, p.idx.data(), sizeof(int) * nnz, hipMemcpyHostToDevice, c->stream));
            HB_HIP(hipMemcpyAsync(dval, p.val.data(), sizeof(double) * (size_t)nnz * RB, hipMemcpyHostToDevice, c->stream));
            HB_HIP(hipMemcpyAsync(dsegs, hsegs.data(), sizeof(int) * hsegs.size(), hipMemcpyHostToDevice, c->stream));
            HB_HIP(hipMemcpyAsync(dshift, hshift.data(), sizeof(double) * hshift.size(), hipMemcpyHostToDevice, c->stream));
            HB_HIP(hipMemcpyAsync(dchunks, hchunks.data(), sizeof(int) * hchunks.size(), hipMemcpyHostToDevice, c->stream));
            HB_HIP(hipMemsetAsync(dout, 0, sizeof(double) * (size_t)(nw + 1) * RB, c->stream)); // (a window that is never visited: 0.0 exactly)
            // launches of consecutive chunks whose partial pairs fit the buffer
            const size_t per_seg = (size_t)nrb * 2 * RB * sizeof(double);
            const size_t fit = std::max<size_t>(1, PART_CAP_BYTES / per_seg);
            for (int k0 = 0; k0 <= nch;) {
                int k1 = k0, nsg = 0;
                while (k1 <= nch && (k1 == k0 || (size_t)(nsg + hchunks[2 * k1 + 1]) <= fit) && k1 - k0 < 65535) nsg += hchunks[2 * k1 + 1], k1++;
                if ((size_t)nsg > part_segs) {
                    if (dpart) { HB_HIP(hipStreamSynchronize(c->stream)); bufs.drop(&dpart); }
                    HB_TRY(bufs.get(&dpart, (size_t)nsg * nrb * 2 * RB));
                    part_segs = (size_t)nsg;
                }
                const int seg_base = hchunks[2 * k0];
                const dim3 grid((unsigned)nrb, (unsigned)(k1 - k0));
                if (c->layout == 64)
                    hipLaunchKernelGGL(k_window_var_real, grid, dim3(256), 0, c->stream, c->Xd, c->ld, n, didx, dval, dsegs, dshift, dchunks, k0, seg_base, dpart);
                else
                    hipLaunchKernelGGL(k_window_var, grid, dim3(256), 0, c->stream, c->X, c->ld, c->layout == 2 ? c->X2 : nullptr, c->ld2 / 4, n, didx, dval, dsegs,
                                       dshift, dchunks, k0, seg_base, dpart);
                HB_HIP(hipGetLastError());
                hipLaunchKernelGGL(k_window_var_fin, dim3((unsigned)((nsg * RB + 255) / 256)), dim3(256), 0, c->stream, dpart, dsegs, seg_base, nsg, nrb, n, dout);
                HB_HIP(hipGetLastError());
                k0 = k1;
            }
            HB_HIP(hipMemcpyAsync(hout.data(), dout, sizeof(double) * hout.size(), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
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

} // extern "C"
