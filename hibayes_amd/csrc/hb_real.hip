// hb_real.hip — the fp64 resident layout (genotype_bits = 64): the sweep's kernels on real-valued genotype columns.
//
// The reference's Bayes() takes any real matrix (arma::mat&); imputed dosages, and the stacked genotyped / imputed rows the single-step
// front-end builds (R/ssbayes.r:305,318), are not integer codes. They are kept as column-major doubles with X's row padding (ld rows,
// zero-filled; m_pad columns) and swept by the event-ordered per-panel route (enqueue_sweep_kernels, hb_kernels.hip) at lag 0, one panel
// per mat-vec, with the diagonal Gram block of each panel only:
//   k_dot_real     partial[split][j] = sum over the split's rows of x[row][j] * yadj[row]     HBM-bound at 8 bytes per genotype (the dominant kernel)
//   k_chain<K1, double>  (hb_chain_panel.hpp)                                                 the same chain, its Gram rows doubles
//   k_update_real  yadj -= sum_e x_e D_e, u += the same, r32 = (float)yadj
// and beside the sweep: k_stats_real (xpx, vx in two passes), k_gram_real (G_p = X_p' X_p on the fp64 matrix cores), k_xalpha_real /
// k_xmat_real (X alpha, the GEBV sample matrix), the finiteness check of an upload and the int8 -> fp64 conversion.
// Everything that sums is deterministic: shuffle trees, row splits added in split order, no floating-point atomics — but k_xalpha_real,
// which keeps k_xalpha's atomics over its column blocks.
// A translation unit of its own: hb_kernels.hip's headline chain sits at the register limit and has spilled before when instantiations
// were added beside it (README, round 6); the Makefile keeps this unit's resource report too (hb_real.res.txt).
#include "hb_internal.hpp"
#include "hb_mma.hpp"

// block-wide sum of 256 threads in a fixed order, valid in every thread; red: 4 doubles. Not hb_wave.hpp's block_sum: the wave sums
// are added as (r0 + r1) + (r2 + r3), not in wave order, and the layout's bit-for-bit tests rest on the sums that order gives.
__device__ __forceinline__ double real_block_sum(double v, double *red)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------------------------------------
// ingest: is every entry finite? / int8 columns -> fp64 columns
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_real_check(const double *__restrict__ X, int64_t count, int *__restrict__ bad)
{
    bool b = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) b |= !(fabs(X[i]) < HB_INF);
    if (__any(b) && (threadIdx.x & 63) == 0) atomicExch(bad, 1);
}

__global__ __launch_bounds__(256) void k_i8_to_real(const int8_t *__restrict__ X, int64_t count, double *__restrict__ Xd)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) Xd[i] = (double)X[i];
}

// ---------------------------------------------------------------------------------------------
// marker statistics (reference src/Bayes.cpp:310-317), one workgroup per column, thread = 2 consecutive rows per step
// xpx = sum x^2; vx = arma::var, two passes: the mean, then the squared deviations with arma's correction term, N - 1 denominator. The
// one-pass N S2 - S1^2 of the integer k_stats is not exact on doubles. A column whose entries are all the same number has vx == 0.0
// exactly (its minimum is its maximum), and is skipped like a monomorphic marker.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_stats_real(const double *__restrict__ X, int64_t ld, int n, int m, double *__restrict__ xpx,
                                                    double *__restrict__ vx, int *__restrict__ xinfo, double *__restrict__ s1out)
{
    __shared__ double red[4];
    __shared__ double ext[2][4];
    const int j = blockIdx.x, tid = threadIdx.x;
    const double *col = X + (int64_t)j * ld;
    double s1 = 0.0, s2 = 0.0, mn = HB_INF, mx = -HB_INF;
    for (int64_t r0 = (int64_t)tid * 2; r0 < ld; r0 += 512) { // (the padding rows hold zeros: only the extremes need the row count)
        const d2 v = *reinterpret_cast<const d2 *>(col + r0);
        s1 += v.x + v.y;
        s2 = fma(v.x, v.x, s2);
        s2 = fma(v.y, v.y, s2);
        if (r0 < n) { mn = fmin(mn, v.x); mx = fmax(mx, v.x); }
        if (r0 + 1 < n) { mn = fmin(mn, v.y); mx = fmax(mx, v.y); }
    }
    s1 = real_block_sum(s1, red);
    s2 = real_block_sum(s2, red);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, o, 64));
        mx = fmax(mx, __shfl_xor(mx, o, 64));
    }
    if ((tid & 63) == 0) { ext[0][tid >> 6] = mn; ext[1][tid >> 6] = mx; }
    __syncthreads();
    mn = fmin(fmin(ext[0][0], ext[0][1]), fmin(ext[0][2], ext[0][3]));
    mx = fmax(fmax(ext[1][0], ext[1][1]), fmax(ext[1][2], ext[1][3]));
    const double mean = s1 / (double)n;
    double a2 = 0.0, a3 = 0.0;
    for (int64_t r0 = (int64_t)tid * 2; r0 < n; r0 += 512) {
        const d2 v = *reinterpret_cast<const d2 *>(col + r0);
        const double t0 = mean - v.x, t1 = (r0 + 1 < n) ? mean - v.y : 0.0;
        a2 = fma(t0, t0, a2);
        a2 = fma(t1, t1, a2);
        a3 += t0 + t1;
    }
    a2 = real_block_sum(a2, red);
    a3 = real_block_sum(a3, red);
    if (tid == 0) {
        if (s1out) s1out[j] = j < m ? s1 : 0.0;
        if (j < m) {
            xpx[j] = s2;
            vx[j] = (mn == mx || n < 2) ? 0.0 : (a2 - a3 * a3 / (double)n) / (double)(n - 1);
            // (the integer bounds of the values: what the int8 layouts keep in xmin / xmax)
            atomicMin(&xinfo[0], (int)fmax(-1073741824.0, floor(mn)));
            atomicMax(&xinfo[1], (int)fmin(1073741824.0, ceil(mx)));
        } else {
            xpx[j] = 0.0;
            vx[j] = 0.0;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_dot_real: partial[split][col] = sum over the split's rows of x[row][col] * yadj[row], fp64 FMA whatever `precise` says
// tile = HBR_CT columns x (256 threads x 2 rows) per step, a split = HBR_CHUNK rows (the context's nsplit = ceil(ld / 4096));
// grid = (ncols / HBR_CT, nsplit). The genotypes are streamed once with 16-byte non-temporal loads, so that the residual stays in L2.
// k_dot's split / partial scheme: the chain (or k_sum_partials) adds the partials in split order, so a product is the same bits from run
// to run and does not depend on which workgroup finishes first.
// ---------------------------------------------------------------------------------------------
#define HBR_CT 8
#define HBR_CHUNK 4096
__global__ __launch_bounds__(256) void k_dot_real(const double *__restrict__ X, int64_t ld, const double *__restrict__ r,
                                                  double *__restrict__ partial, int pstride)
{
    __shared__ double red[4][HBR_CT];
    const int ct = blockIdx.x, sp = blockIdx.y, tid = threadIdx.x;
    const double *xc = X + (int64_t)ct * HBR_CT * ld;
    double acc[HBR_CT];
#pragma unroll
    for (int c = 0; c < HBR_CT; c++) acc[c] = 0.0;
    const int64_t row1 = (int64_t)(sp + 1) * HBR_CHUNK < ld ? (int64_t)(sp + 1) * HBR_CHUNK : ld;
#pragma unroll 2
    for (int64_t row0 = (int64_t)sp * HBR_CHUNK + tid * 2; row0 < row1; row0 += 512) { // (ld is a multiple of 256: a pair of rows is inside or outside)
        d2 xv[HBR_CT];
#pragma unroll
        for (int c = 0; c < HBR_CT; c++) xv[c] = __builtin_nontemporal_load(reinterpret_cast<const d2 *>(xc + (int64_t)c * ld + row0));
        const d2 rv = *reinterpret_cast<const d2 *>(r + row0);
#pragma unroll
        for (int c = 0; c < HBR_CT; c++) {
            acc[c] = fma(xv[c].x, rv.x, acc[c]);
            acc[c] = fma(xv[c].y, rv.y, acc[c]);
        }
    }
    const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int c = 0; c < HBR_CT; c++) {
        const double s = wave_sum(acc[c]);
        if (lane == 0) red[wv][c] = s;
    }
    __syncthreads();
    if (tid < HBR_CT) partial[(int64_t)sp * pstride + ct * HBR_CT + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// ---------------------------------------------------------------------------------------------
// k_gram_real: the diagonal Gram block G_p = X_p' X_p of every panel in fp64 on the matrix cores (v_mfma_f64_16x16x4_f64, hb_mma.hpp).
// One wave = one 32 x 32 tile (bi >= bj) of the lower triangle of panel blockIdx.y's P x P block, over all ld rows in one fixed order
// (no row split, no atomics: the block is the same bits from build to build). A lane reads 16 bytes of its column per step — rows
// 2 (lane >> 4) and 2 (lane >> 4) + 1 of the step's 8 — and gives the even rows to one MFMA step and the odd rows to the next: both
// operands number the four k values of a step by lane >> 4, which is all the instruction asks.
// k_gram_real_finish mirrors the lower triangle into the upper one and stores xpx on the diagonal: the number the chain uses as xpx[j]
// and the stored G[j][j] are then one number, not two sums that can differ in the last bit.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gram_real(const double *__restrict__ X, int64_t ld, int P, int ntiles, double *__restrict__ G)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + wave;
    if (t >= ntiles) return; // (wave-uniform)
    int bi, bj;
    tri_tile(t, &bi, &bj);
    const int p = blockIdx.y;
    const double *Xp = X + (int64_t)p * P * ld;
    const double *xa = Xp + (int64_t)(32 * bi + (lane & 15)) * ld + 2 * (lane >> 4); // rows of G
    const double *ya = Xp + (int64_t)(32 * bj + (lane & 15)) * ld + 2 * (lane >> 4); // columns of G
    v4d acc[2][2];
    mma_f64_zero(acc);
    for (int64_t k = 0; k < ld; k += 8) {
        d2 x[2], y[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            x[h] = *reinterpret_cast<const d2 *>(xa + (int64_t)16 * h * ld + k);
            y[h] = *reinterpret_cast<const d2 *>(ya + (int64_t)16 * h * ld + k);
        }
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++) {
                acc[a][b] = mfma_f64(x[b].x, y[a].x, acc[a][b]);
                acc[a][b] = mfma_f64(x[b].y, y[a].y, acc[a][b]);
            }
    }
    double *Gp = G + (size_t)p * P * P;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                Gp[(size_t)(32 * bi + mma_f64_row(b, r, lane)) * P + 32 * bj + mma_f64_col(a, lane)] = acc[a][b][r];
}

__global__ __launch_bounds__(256) void k_gram_real_finish(double *__restrict__ G, int P, const double *__restrict__ xpx)
{
    const int p = blockIdx.y;
    double *Gp = G + (size_t)p * P * P;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < P * P; e += gridDim.x * blockDim.x) {
        const int i = e / P, j = e - i * P;
        if (i < j) Gp[e] = Gp[(size_t)j * P + i]; // (the tiles on the diagonal wrote their upper halves too: overwritten by the same product's other order)
        else if (i == j) Gp[e] = xpx[(size_t)p * P + i];
    }
}

// ---------------------------------------------------------------------------------------------
// k_update_real: yadj -= sum_e x_e D_e, u += the same, r32 = (float)yadj for panel p's changed markers (a kernel boundary separates it
// from the chain that wrote the move list). thread = 2 consecutive rows; the list is staged in LDS once, then the column loads of 8 moves
// are in flight together. The moves are applied in list order, as update_rows applies them.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_update_real(const double *__restrict__ X, int64_t ld, int P, int p, const int32_t *__restrict__ ev_count,
                                                     const int32_t *__restrict__ ev_idx, const double *__restrict__ ev_delta,
                                                     double *__restrict__ r, double *__restrict__ u, float *__restrict__ r32)
{
    __shared__ int s_ix[512];
    __shared__ double s_dl[512 + 8];
    const int nev = min(ev_count[(size_t)p * HB_EVS], min(P, 512));
    if (nev <= 0) return; // (uniform: nothing moved, the residual stands)
    for (int e = threadIdx.x; e < nev + 8; e += blockDim.x) {
        s_ix[min(e, 511)] = ev_idx[(size_t)p * P + min(e, nev - 1)] & (P - 1);
        s_dl[e] = e < nev ? ev_delta[(size_t)p * P + e] : 0.0; // (zero past the list: a batch reads past it without a test per move)
    }
    __syncthreads();
    const int64_t row0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
    if (row0 >= ld) return;
    const double *Xp = X + (int64_t)p * P * ld + row0;
    double a0 = 0.0, a1 = 0.0;
    for (int e0 = 0; e0 < nev; e0 += 8) {
        d2 w[8];
#pragma unroll
        for (int k = 0; k < 8; k++) w[k] = *reinterpret_cast<const d2 *>(Xp + (int64_t)s_ix[min(e0 + k, nev - 1)] * ld);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const double d = s_dl[e0 + k];
            a0 = fma(w[k].x, d, a0);
            a1 = fma(w[k].y, d, a1);
        }
    }
    d2 rv = *reinterpret_cast<const d2 *>(r + row0), uv = *reinterpret_cast<const d2 *>(u + row0);
    rv.x -= a0; rv.y -= a1;
    uv.x += a0; uv.y += a1;
    *reinterpret_cast<d2 *>(r + row0) = rv;
    *reinterpret_cast<d2 *>(u + row0) = uv;
    *reinterpret_cast<float2 *>(r32 + row0) = make_float2((float)rv.x, (float)rv.y);
}

// ---------------------------------------------------------------------------------------------
// egress: out[row] = sum_j x[row][j] alpha[j] (e, g; reference src/Bayes.cpp:971) and the GEBV sample matrix, eight records per pass
// over the columns that carry an effect (R/bayes.r:303-305): k_xalpha / k_xmat (hb_ingest.hpp) on fp64 columns, thread = 2 rows
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_xalpha_real(const double *__restrict__ X, int64_t ld, int m_pad, const double *__restrict__ alpha,
                                                     double *__restrict__ out)
{
    const int64_t row0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
    if (row0 >= ld) return;
    const int j0 = blockIdx.y * 256, j1 = min(m_pad, j0 + 256);
    double a0 = 0.0, a1 = 0.0;
    for (int j = j0; j < j1; j++) {
        const double al = alpha[j];
        if (al == 0.0) continue;
        const d2 w = *reinterpret_cast<const d2 *>(X + (int64_t)j * ld + row0);
        a0 = fma(w.x, al, a0);
        a1 = fma(w.y, al, a1);
    }
    if (a0 != 0.0) atomicAdd(out + row0, a0);
    if (a1 != 0.0) atomicAdd(out + row0 + 1, a1);
}

#define HBR_XM_RB 8 // (hb_ctx_matmul's RB)
__global__ __launch_bounds__(256) void k_xmat_real(const double *__restrict__ X, int64_t ld, const int *__restrict__ idx, const double *__restrict__ val,
                                                   int nnz, double *__restrict__ out, int64_t ldo)
{
    const int64_t row0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
    if (row0 >= ld) return;
    double acc[2][HBR_XM_RB];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int rr = 0; rr < HBR_XM_RB; rr++) acc[a][rr] = 0.0;
    for (int e0 = 0; e0 < nnz; e0 += 4) {
        d2 w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = *reinterpret_cast<const d2 *>(X + (int64_t)idx[min(e0 + k, nnz - 1)] * ld + row0);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (e0 + k < nnz) { // uniform
                const double *v = val + (size_t)(e0 + k) * HBR_XM_RB;
#pragma unroll
                for (int rr = 0; rr < HBR_XM_RB; rr++) {
                    acc[0][rr] = fma(w[k].x, v[rr], acc[0][rr]);
                    acc[1][rr] = fma(w[k].y, v[rr], acc[1][rr]);
                }
            }
        }
    }
#pragma unroll
    for (int rr = 0; rr < HBR_XM_RB; rr++) {
        out[(int64_t)rr * ldo + row0] = acc[0][rr];
        out[(int64_t)rr * ldo + row0 + 1] = acc[1][rr];
    }
}

// =============================================================================================
// host side: launchers
// =============================================================================================
static unsigned grid_for(int64_t count, const hb_ctx *c) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((count + 255) / 256, (int64_t)c->num_cus * 8)); }

int hbk_real_check(hb_ctx *c, int *bad)
{
    int *dbad = reinterpret_cast<int *>(c->scratch);
    HB_HIP(hipMemsetAsync(dbad, 0, sizeof(int), c->stream));
    const int64_t count = c->ld * (int64_t)c->m_pad;
    hipLaunchKernelGGL(k_real_check, dim3(grid_for(count, c)), dim3(256), 0, c->stream, c->Xd, count, dbad);
    HB_HIP(hipGetLastError());
    HB_HIP(hipMemcpyAsync(bad, dbad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    return HB_OK;
}

int hbk_real_from_i8(hb_ctx *c)
{
    const int64_t count = c->ld * (int64_t)c->m_pad;
    hipLaunchKernelGGL(k_i8_to_real, dim3(grid_for(count, c)), dim3(256), 0, c->stream, c->X, count, c->Xd);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_real_stats(hb_ctx *c)
{
    int init[2] = {1073741824, -1073741824};
    HB_HIP(hipMemcpyAsync(c->xinfo, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_stats_real, dim3(c->m_pad), dim3(256), 0, c->stream, c->Xd, c->ld, c->n, c->m, c->xpx, c->vx, c->xinfo, c->s1);
    HB_HIP(hipGetLastError());
    int info[2];
    HB_HIP(hipMemcpyAsync(info, c->xinfo, sizeof(info), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    c->xmin = info[0];
    c->xmax = info[1];
    c->stats_ready = true;
    return HB_OK;
}

int hbk_real_dot(hb_ctx *c, int col0, int ncols, const double *r, hipStream_t st)
{
    if (col0 < 0 || ncols <= 0 || ncols % HBR_CT || col0 + ncols > c->m_pad || (int64_t)c->nsplit * HBR_CHUNK < c->ld)
        return hb_fail(HB_ERR_INVALID, "k_dot_real: columns outside the padded matrix, or row splits that do not cover it");
    hipLaunchKernelGGL(k_dot_real, dim3(ncols / HBR_CT, c->nsplit), dim3(256), 0, st ? st : c->stream, c->Xd + (int64_t)col0 * c->ld, c->ld, r,
                       c->partial + col0, c->m_pad);
    return HB_OK;
}

int hbk_real_gram(hb_ctx *c)
{
    if (c->P % 32) return hb_fail(HB_ERR_INVALID, "k_gram_real: the panel must be a multiple of 32");
    const int T = c->P / 32, ntiles = T * (T + 1) / 2;
    hipLaunchKernelGGL(k_gram_real, dim3((ntiles + 3) / 4, c->npanels), dim3(256), 0, c->stream, c->Xd, c->ld, c->P, ntiles, c->gramd);
    hipLaunchKernelGGL(k_gram_real_finish, dim3(std::min(64, (c->P * c->P + 255) / 256), c->npanels), dim3(256), 0, c->stream, c->gramd, c->P, c->xpx);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_real_update(hb_ctx *c, int p, double *r, float *r32, hipStream_t st)
{
    if (p < 0 || p >= c->npanels) return hb_fail(HB_ERR_INVALID, "k_update_real: no such panel");
    hipLaunchKernelGGL(k_update_real, dim3((unsigned)((c->ld / 2 + 255) / 256)), dim3(256), 0, st ? st : c->stream, c->Xd, c->ld, c->P, p, c->ev_count,
                       c->ev_idx, c->ev_delta, r, c->u, r32);
    return HB_OK;
}

int hbk_real_xalpha(hb_ctx *c, const double *dev_alpha, double *dev_out)
{
    const dim3 grid((unsigned)((c->ld / 2 + 255) / 256), (unsigned)((c->m_pad + 255) / 256));
    hipLaunchKernelGGL(k_xalpha_real, grid, dim3(256), 0, c->stream, c->Xd, c->ld, c->m_pad, dev_alpha, dev_out);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_real_xmat(hb_ctx *c, const int *didx, const double *dval, int nnz, double *dout)
{
    hipLaunchKernelGGL(k_xmat_real, dim3((unsigned)((c->ld / 2 + 255) / 256)), dim3(256), 0, c->stream, c->Xd, c->ld, didx, dval, nnz, dout, c->ld);
    HB_HIP(hipGetLastError());
    return HB_OK;
}
