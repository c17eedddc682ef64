// hb_epsl.hip — the epsilon block of the single-step model (reference src/Bayes.cpp:554-584, Gibbs(sp_mat) src/solver.cpp:131-140) on the
// device. A unit of its own, compiled without floating-point contraction: every expression below rounds as it is written, and
// tests/epsl_restatement.py writes the same ones.
//
// One step, enqueued on the context's stream with no host synchronisation:
//     k_epsl_chunkdot  partial sums of y_J . yadj over fixed chunks of 256 rows (a fixed tree inside a chunk)
//     k_epsl_jfin      rhs = the partials in chunk order; J_new = (rhs + JtJ J_old) / JtJ + sqrt(vare / JtJ) zJ          (:555-559)
//     k_epsl_japply    yadj += (J_old - J_new) y_J, u -= the same, the fp32 image of yadj                                   (:560-563)
//     k_epsl_b         b_i = (sum of yadj over the records of individual i, in record order, from 0) + zz_i x_i; x_old = x  (:567-569)
//     k_epsl_narrow / k_epsl_wide, as hb_epslplan.hpp lists them: the rows of the pass, level by level                      (:570)
//     k_epsl_scatter   yadj_tail[r] += x_old[idx_r] - x[idx_r], u_tail[r] -= the same, the fp32 image                       (:572-576)
//     k_epsl_gx        t_i = sum_j G_ji x_j, then k_epsl_chunkdot(x, t) and
//     k_epsl_vfin      q = x'Gx = the partials in chunk order, veps = (q + s2_df) / chis                                    (:577-579)
// A row of the pass, whatever launch, lane or wave evaluates it (epsl_row):
//     lam  = vare / veps
//     s    = 0; for the stored entries k of column i in ascending row index j (the diagonal among them): s = s + G_k * x_j
//     a_ii = zz_i + lam * G_ii
//     Ax   = zz_i * x_i + lam * s
//     x_i  = ((b_i - Ax) / a_ii + x_i) + sqrt(vare / a_ii) * z_i,   z_i = the normal of Philox purpose 6, blk = i (hb_rng.hpp)
// A wave loads 64 entries of the column at once and then adds the 64 products in the same ascending order, every lane the same chain: the sum
// is the lane's, bit for bit. No floating-point atomic anywhere and no kernel waits for another workgroup.
#include "hb_internal.hpp"
#include "hb_rng.hpp"
#include "hb_epslplan.hpp"
#include <cmath>
#include <cstring>

struct hb_epsl {
    int q = 0, ne = 0, n = 0, tail0 = 0;
    int64_t nnz = 0;
    int64_t *indptr = nullptr;
    int32_t *indices = nullptr, *rec_ptr = nullptr, *rec = nullptr, *idx = nullptr, *rows = nullptr, *steps = nullptr;
    double *data = nullptr, *diag = nullptr, *zz = nullptr, *yJ = nullptr, *x = nullptr, *xold = nullptr, *b = nullptr, *t = nullptr, *xsum = nullptr,
           *parts = nullptr;
    double *st = nullptr;   // device: [0] veps, [1] q = x'Gx, [2] J, [3] rhs of the J draw, [4] J_old - J_new
    double *h_st = nullptr; // pinned mirror, filled by the sweep's fetch
    double JtJ = 0;
    int steps_cap = 0;
    int sched_mode = 0, row_mode = 0;
    int stored = 0;
    std::vector<int64_t> h_indptr; // the pattern, kept for a change of plan (hb_ctx_epsl_debug_set)
    std::vector<int32_t> h_indices;
    hb_epsl_sched plan;
    hb_bufs mem; // every device and pinned buffer above
};

namespace {

constexpr int ET = 256;

struct epsl_view {
    const int64_t *indptr;
    const int32_t *indices;
    const double *data, *diag, *zz, *b;
    double *x; // read and written inside one launch: never __restrict__
    const int32_t *rows, *steps;
    const double *st;
    double vare, veps_in;
    uint64_t seed, sub;
    int q;
};

__device__ __forceinline__ double epsl_row(double s, double xi, double bi, double zz, double gii, double lam, double vare, double z)
{
    const double aii = zz + lam * gii;
    const double Ax = zz * xi + lam * s;
    return ((bi - Ax) / aii + xi) + sqrt(vare / aii) * z;
}

__device__ __forceinline__ double epsl_lam(const epsl_view &v) { return v.vare / (v.veps_in >= 0.0 ? v.veps_in : v.st[0]); }

__device__ __forceinline__ void epsl_lane_row(const epsl_view &v, int i, double lam)
{
    double s = 0.0;
    for (int64_t k = v.indptr[i]; k < v.indptr[i + 1]; k++) s = s + v.data[k] * v.x[v.indices[k]];
    const double z = hb_normal_blk(v.seed, v.sub, (uint64_t)i);
    v.x[i] = epsl_row(s, v.x[i], v.b[i], v.zz[i], v.diag[i], lam, v.vare, z);
}

// lane l's value to every lane of the wave; l is wave-uniform (a scalar register): two v_readlane_b32, no trip through the LDS crossbar
__device__ __forceinline__ double epsl_bcast(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// all 64 lanes of the wave call it with the same i
__device__ __forceinline__ void epsl_wave_row(const epsl_view &v, int i, double lam, int lane)
{
    const int64_t k0 = v.indptr[i], k1 = v.indptr[i + 1];
    double s = 0.0;
    for (int64_t base = k0; base < k1; base += 64) {
        const int64_t k = base + lane;
        double g = 0.0, xv = 0.0;
        if (k < k1) {
            g = v.data[k];
            xv = v.x[v.indices[k]];
        }
        const int cnt = __builtin_amdgcn_readfirstlane((int)(k1 - base < 64 ? k1 - base : 64)); // (the same in every lane: a scalar loop)
        for (int l = 0; l < cnt; l++) s = s + epsl_bcast(g, l) * epsl_bcast(xv, l);
    }
    const double xi = v.x[i];
    if (lane == 0) {
        const double z = hb_normal_blk(v.seed, v.sub, (uint64_t)i);
        v.x[i] = epsl_row(s, xi, v.b[i], v.zz[i], v.diag[i], lam, v.vare, z);
    }
}

// one workgroup, steps [s0, s1): the rows of a step, a barrier, the next step
__global__ __launch_bounds__(ET) void k_epsl_narrow(epsl_view v, int s0, int s1)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double lam = epsl_lam(v);
    for (int s = s0; s < s1; s++) {
        const int32_t *sp = v.steps + 5 * s;
        const int lane0 = sp[1], nlane = sp[2], wave0 = sp[3], nwave = sp[4];
        for (int t = threadIdx.x; t < nlane; t += ET) epsl_lane_row(v, v.rows[lane0 + t], lam);
        for (int w = wave; w < nwave; w += ET / 64) epsl_wave_row(v, v.rows[wave0 + w], lam, lane);
        __syncthreads();
    }
}

// step s over the chip: workgroups [0, nb_lane) take 256 lane rows each, the others four wave rows each
__global__ __launch_bounds__(ET) void k_epsl_wide(epsl_view v, int s, int nb_lane)
{
    const int32_t *sp = v.steps + 5 * s;
    const int lane0 = sp[1], nlane = sp[2], wave0 = sp[3], nwave = sp[4];
    const double lam = epsl_lam(v);
    if ((int)blockIdx.x < nb_lane) {
        const int t = blockIdx.x * ET + threadIdx.x;
        if (t < nlane) epsl_lane_row(v, v.rows[lane0 + t], lam);
    } else {
        const int w = ((int)blockIdx.x - nb_lane) * (ET / 64) + (threadIdx.x >> 6);
        if (w < nwave) epsl_wave_row(v, v.rows[wave0 + w], lam, threadIdx.x & 63); // (uniform in the wave)
    }
}

// parts[chunk] = sum over the chunk's 256 rows of a_i b_i: the products in a fixed tree
__global__ __launch_bounds__(ET) void k_epsl_chunkdot(const double *__restrict__ a, const double *__restrict__ b, int n, double *__restrict__ parts)
{
    __shared__ double red[ET];
    const int i = blockIdx.x * ET + threadIdx.x;
    red[threadIdx.x] = i < n ? a[i] * b[i] : 0.0;
    __syncthreads();
    for (int o = ET / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) parts[blockIdx.x] = red[0];
}

// the partials in chunk order, from 0: tiles of 256 through LDS, thread 0 adds (one workgroup)
__device__ __forceinline__ double epsl_seq_sum(const double *__restrict__ parts, int nch, double *tile)
{
    double s = 0.0;
    for (int c0 = 0; c0 < nch; c0 += ET) {
        const int c = c0 + threadIdx.x;
        tile[threadIdx.x] = c < nch ? parts[c] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = nch - c0 < ET ? nch - c0 : ET;
            for (int l = 0; l < cnt; l++) s = s + tile[l];
        }
        __syncthreads();
    }
    return s; // (thread 0's)
}

__global__ __launch_bounds__(ET) void k_epsl_jfin(const double *__restrict__ parts, int nch, double *__restrict__ st, double JtJ, double vare, double zJ)
{
    __shared__ double tile[ET];
    double rhs = epsl_seq_sum(parts, nch, tile);
    if (threadIdx.x == 0) {
        const double old = st[2];
        st[3] = rhs;
        rhs = rhs + JtJ * old;
        const double gi = rhs / JtJ + sqrt(vare / JtJ) * zJ;
        st[2] = gi;
        st[4] = old - gi;
    }
}

__global__ __launch_bounds__(ET) void k_epsl_japply(double *__restrict__ r, float *__restrict__ r32, double *__restrict__ u, const double *__restrict__ yJ, int n,
                                                    const double *__restrict__ st)
{
    const int i = blockIdx.x * ET + threadIdx.x;
    if (i >= n) return;
    const double d = st[4] * yJ[i];
    const double v = r[i] + d;
    r[i] = v;
    r32[i] = (float)v;
    u[i] = u[i] - d;
}

__global__ __launch_bounds__(ET) void k_epsl_b(const double *__restrict__ rt, const int32_t *__restrict__ rec_ptr, const int32_t *__restrict__ rec,
                                               const double *__restrict__ zz, const double *__restrict__ x, double *__restrict__ xold, double *__restrict__ b, int q)
{
    const int i = blockIdx.x * ET + threadIdx.x;
    if (i >= q) return;
    double s = 0.0;
    for (int p = rec_ptr[i]; p < rec_ptr[i + 1]; p++) s = s + rt[rec[p]];
    const double xi = x[i];
    b[i] = s + zz[i] * xi;
    xold[i] = xi;
}

__global__ __launch_bounds__(ET) void k_epsl_scatter(double *__restrict__ rt, float *__restrict__ rt32, double *__restrict__ ut, const int32_t *__restrict__ idx,
                                                     const double *__restrict__ xold, const double *__restrict__ x, int ne)
{
    const int r = blockIdx.x * ET + threadIdx.x;
    if (r >= ne) return;
    const int i = idx[r];
    const double d = xold[i] - x[i];
    const double v = rt[r] + d;
    rt[r] = v;
    rt32[r] = (float)v;
    ut[r] = ut[r] - d;
}

__global__ __launch_bounds__(ET) void k_epsl_gx(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const double *__restrict__ data,
                                                const double *__restrict__ x, double *__restrict__ t, int q)
{
    const int i = blockIdx.x * ET + threadIdx.x;
    if (i >= q) return;
    double s = 0.0;
    for (int64_t k = indptr[i]; k < indptr[i + 1]; k++) s = s + data[k] * x[indices[k]];
    t[i] = s;
}

__global__ __launch_bounds__(ET) void k_epsl_vfin(const double *__restrict__ parts, int nch, double *__restrict__ st, double s2_df, double chis)
{
    __shared__ double tile[ET];
    const double qv = epsl_seq_sum(parts, nch, tile);
    if (threadIdx.x == 0) {
        st[1] = qv;
        st[0] = (qv + s2_df) / chis;
    }
}

__global__ __launch_bounds__(ET) void k_epsl_add(double *__restrict__ y, const double *__restrict__ x, int n)
{
    const int i = blockIdx.x * ET + threadIdx.x;
    if (i < n) y[i] = y[i] + x[i];
}

int epsl_check(hb_ctx *c, const char *who)
{
    if (!c) return hb_fail(HB_ERR_INVALID, std::string(who) + ": null context");
    if (!c->epsl) return hb_fail(HB_ERR_INVALID, std::string(who) + ": call hb_ctx_epsl_setup first");
    HB_HIP(hipSetDevice(c->device));
    return HB_OK;
}

unsigned blocks(int n) { return (unsigned)((n + ET - 1) / ET); }

// the plan for the current modes, rows and steps to the device (synchronises: the tables may be in use)
int epsl_plan_upload(hb_ctx *c)
{
    hb_epsl *p = c->epsl;
    HB_HIP(hipStreamSynchronize(c->stream));
    p->plan = hb_epsl_plan_of(p->q, p->h_indptr.data(), p->h_indices.data(), p->sched_mode, p->row_mode);
    const int ns = (int)p->plan.steps.size();
    if (ns > p->steps_cap) return hb_fail(HB_ERR_INVALID, "hb_epsl: more steps than rows");
    std::vector<int32_t> st((size_t)5 * std::max(ns, 1));
    for (int s = 0; s < ns; s++) {
        const hb_epsl_step &e = p->plan.steps[s];
        const int32_t v[5] = {e.level, e.lane0, e.nlane, e.wave0, e.nwave};
        std::memcpy(&st[(size_t)5 * s], v, sizeof v);
    }
    HB_HIP(hipMemcpy(p->rows, p->plan.rows.data(), sizeof(int32_t) * (size_t)p->q, hipMemcpyHostToDevice));
    HB_HIP(hipMemcpy(p->steps, st.data(), sizeof(int32_t) * (size_t)5 * ns, hipMemcpyHostToDevice));
    return HB_OK;
}

} // namespace

void hb_epsl_free(hb_ctx *c)
{
    hb_epsl *p = c ? c->epsl : nullptr;
    if (!p) return;
    delete p;
    c->epsl = nullptr;
}

// veps, q, J ride on the sweep's fetch (fetch_acc, hb_ctx.hip): no host synchronisation of their own
int hb_epsl_fetch_enqueue(hb_ctx *c)
{
    hb_epsl *p = c->epsl;
    if (!p) return HB_OK;
    HB_HIP(hipMemcpyAsync(p->h_st, p->st, sizeof(double) * 8, hipMemcpyDeviceToHost, c->stream));
    return HB_OK;
}

const double *hb_epsl_host_state(const hb_ctx *c) { return c && c->epsl ? c->epsl->h_st : nullptr; }
int hb_epsl_q(const hb_ctx *c) { return c && c->epsl ? c->epsl->q : 0; }
int hb_epsl_ne(const hb_ctx *c) { return c && c->epsl ? c->epsl->ne : 0; }

// epsilon = 0, J = 0, no records: a run starts (:251, :268-269)
int hb_epsl_reset(hb_ctx *c)
{
    int rc = epsl_check(c, "hb_epsl_reset");
    if (rc) return rc;
    hb_epsl *p = c->epsl;
    const size_t vl = sizeof(double) * (size_t)p->q;
    HB_HIP(hipMemsetAsync(p->x, 0, vl, c->stream));
    HB_HIP(hipMemsetAsync(p->xold, 0, vl, c->stream));
    HB_HIP(hipMemsetAsync(p->xsum, 0, vl, c->stream));
    HB_HIP(hipMemsetAsync(p->st, 0, sizeof(double) * 8, c->stream));
    p->stored = 0;
    return HB_OK;
}

// the thinned store of :876: the running sum, and the record itself where the caller wants it (host, q doubles; synchronises then)
int hbk_epsl_accumulate(hb_ctx *c, double *record)
{
    int rc = epsl_check(c, "hbk_epsl_accumulate");
    if (rc) return rc;
    hb_epsl *p = c->epsl;
    hipLaunchKernelGGL(k_epsl_add, dim3(blocks(p->q)), dim3(ET), 0, c->stream, p->xsum, p->x, p->q);
    HB_HIP(hipGetLastError());
    p->stored++;
    if (record) {
        HB_HIP(hipMemcpyAsync(record, p->x, sizeof(double) * (size_t)p->q, hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
    }
    return HB_OK;
}

// the running sum of the records (q doubles, host) and the individual of each tail record, 0-based (ne, host); either may be NULL
int hbk_epsl_sum(hb_ctx *c, double *xsum, int32_t *idx)
{
    int rc = epsl_check(c, "hbk_epsl_sum");
    if (rc) return rc;
    hb_epsl *p = c->epsl;
    if (xsum) HB_HIP(hipMemcpyAsync(xsum, p->xsum, sizeof(double) * (size_t)p->q, hipMemcpyDeviceToHost, c->stream));
    if (idx) HB_HIP(hipMemcpyAsync(idx, p->idx, sizeof(int32_t) * (size_t)p->ne, hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    return HB_OK;
}

extern "C" {

int hb_epsl_check(const hb_epsl_gi *Gi, const uint32_t *index, int32_t n)
{
    if (!Gi) return hb_fail(HB_ERR_INVALID, "variance-covariance matrix should be provided for epsilon term.");
    const std::string err = hb_epsl_check_args(Gi->q, Gi->ne, Gi->indptr, Gi->indices, Gi->data, index, n);
    if (!err.empty()) return hb_fail(HB_ERR_INVALID, err);
    return HB_OK;
}

int hb_epsl_plan(int32_t q, const int64_t *indptr, const int32_t *indices, int32_t sched_mode, int32_t row_mode, int32_t *level, int32_t *rows,
                 int32_t *steps, int32_t *launches, int32_t *counts)
{
    if (q < 1 || !indptr || !indices || !counts) return hb_fail(HB_ERR_INVALID, "hb_epsl_plan: null argument");
    if (sched_mode < 0 || sched_mode > 2 || row_mode < 0 || row_mode > 2) return hb_fail(HB_ERR_INVALID, "hb_epsl_plan: modes are 0, 1 or 2");
    for (int32_t i = 0; i < q; i++)
        for (int64_t k = indptr[i]; k < indptr[i + 1]; k++)
            if (indices[k] < 0 || indices[k] >= q) return hb_fail(HB_ERR_INVALID, "hb_epsl_plan: a row index is outside 0 .. q - 1");
    const hb_epsl_sched p = hb_epsl_plan_of(q, indptr, indices, sched_mode, row_mode);
    if (level) std::memcpy(level, p.level.data(), sizeof(int32_t) * (size_t)q);
    if (rows) std::memcpy(rows, p.rows.data(), sizeof(int32_t) * (size_t)q);
    if (steps)
        for (size_t s = 0; s < p.steps.size(); s++) {
            const hb_epsl_step &e = p.steps[s];
            const int32_t v[5] = {e.level, e.lane0, e.nlane, e.wave0, e.nwave};
            std::memcpy(steps + 5 * s, v, sizeof v);
        }
    if (launches)
        for (size_t l = 0; l < p.launches.size(); l++) {
            const int32_t v[3] = {p.launches[l].kind, p.launches[l].s0, p.launches[l].s1};
            std::memcpy(launches + 3 * l, v, sizeof v);
        }
    counts[0] = (int32_t)p.steps.size();
    counts[1] = (int32_t)p.launches.size();
    counts[2] = p.levels;
    counts[3] = p.max_col;
    return HB_OK;
}

int hb_ctx_epsl_setup(hb_ctx *c, const hb_epsl_desc *d)
{
    if (!c) return hb_fail(HB_ERR_INVALID, "hb_ctx_epsl_setup: null context");
    HB_HIP(hipSetDevice(c->device));
    if (c->stream) HB_HIP(hipStreamSynchronize(c->stream));
    hb_epsl_free(c);
    if (!d) return HB_OK; // (drops the block)
    if (!d->Gi) return hb_fail(HB_ERR_INVALID, "variance-covariance matrix should be provided for epsilon term.");
    if (!d->index || !d->y_J) return hb_fail(HB_ERR_INVALID, "hb_ctx_epsl_setup: epsl_y_J, epsl_Gi and epsl_index go together");
    const int n = c->n;
    int rc = hb_epsl_check(d->Gi, d->index, n);
    if (rc) return rc;
    const hb_epsl_gi &G = *d->Gi;
    const int q = G.q, ne = G.ne;
    const int64_t nnz = G.indptr[q];
    double JtJ = 0.0;
    for (int i = 0; i < n; i++) {
        if (!std::isfinite(d->y_J[i])) return hb_fail(HB_ERR_INVALID, "epsl_y_J: a value is not finite");
        JtJ = JtJ + d->y_J[i] * d->y_J[i];
    }
    if (!(JtJ > 0.0)) return hb_fail(HB_ERR_INVALID, "epsl_y_J: the J covariate is zero everywhere");

    hb_epsl *p = new hb_epsl();
    c->epsl = p;
    p->q = q;
    p->ne = ne;
    p->n = n;
    p->tail0 = n - ne;
    p->nnz = nnz;
    p->JtJ = JtJ;
    p->h_indptr.assign(G.indptr, G.indptr + q + 1);
    p->h_indices.assign(G.indices, G.indices + nnz);
    // the records of each individual, in record order; zz = their number
    std::vector<int32_t> rec_ptr(q + 1, 0), rec(ne), idx(ne);
    std::vector<double> zz(q, 0.0), diag(q, 0.0);
    for (int r = 0; r < ne; r++) {
        idx[r] = (int32_t)d->index[r] - 1;
        rec_ptr[idx[r] + 1]++;
    }
    for (int i = 0; i < q; i++) {
        zz[i] = (double)rec_ptr[i + 1];
        rec_ptr[i + 1] += rec_ptr[i];
    }
    {
        std::vector<int32_t> at(rec_ptr.begin(), rec_ptr.end() - 1);
        for (int r = 0; r < ne; r++) rec[at[idx[r]]++] = r;
    }
    for (int i = 0; i < q; i++)
        for (int64_t k = G.indptr[i]; k < G.indptr[i + 1]; k++)
            if (G.indices[k] == i) diag[i] = G.data[k];

    const size_t nch = (size_t)std::max((n + ET - 1) / ET, (q + ET - 1) / ET);
    p->steps_cap = q;
    auto build = [&]() -> int {
        hb_bufs &M = p->mem;
        HB_TRY(M.get(&p->indptr, (size_t)(q + 1)));
        HB_TRY(M.get(&p->indices, (size_t)nnz));
        HB_TRY(M.get(&p->data, (size_t)nnz));
        HB_TRY(M.get(&p->rec_ptr, (size_t)(q + 1)));
        HB_TRY(M.get(&p->rec, (size_t)ne));
        HB_TRY(M.get(&p->idx, (size_t)ne));
        HB_TRY(M.get(&p->rows, (size_t)q));
        HB_TRY(M.get(&p->steps, (size_t)5 * (size_t)p->steps_cap));
        HB_TRY(M.get(&p->yJ, (size_t)n));
        HB_TRY(M.get(&p->parts, nch));
        // (zeroed on the null stream, like the copies behind them: those return after them)
        double **vecs[] = {&p->diag, &p->zz, &p->x, &p->xold, &p->b, &p->t, &p->xsum};
        for (double **v : vecs) HB_TRY(M.zeroed(v, (size_t)q, nullptr));
        HB_TRY(M.zeroed(&p->st, 8, nullptr));
        HB_TRY(M.pin(&p->h_st, 8));
        std::memset(p->h_st, 0, sizeof(double) * 8);
        HB_HIP(hipMemcpy(p->indptr, G.indptr, sizeof(int64_t) * (size_t)(q + 1), hipMemcpyHostToDevice));
        HB_HIP(hipMemcpy(p->indices, G.indices, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice));
        HB_HIP(hipMemcpy(p->data, G.data, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice));
        HB_HIP(hipMemcpy(p->rec_ptr, rec_ptr.data(), sizeof(int32_t) * (size_t)(q + 1), hipMemcpyHostToDevice));
        HB_HIP(hipMemcpy(p->rec, rec.data(), sizeof(int32_t) * (size_t)ne, hipMemcpyHostToDevice));
        HB_HIP(hipMemcpy(p->idx, idx.data(), sizeof(int32_t) * (size_t)ne, hipMemcpyHostToDevice));
        HB_HIP(hipMemcpy(p->diag, diag.data(), sizeof(double) * (size_t)q, hipMemcpyHostToDevice));
        HB_HIP(hipMemcpy(p->zz, zz.data(), sizeof(double) * (size_t)q, hipMemcpyHostToDevice));
        HB_HIP(hipMemcpy(p->yJ, d->y_J, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
        return epsl_plan_upload(c);
    };
    rc = build();
    if (rc) hb_epsl_free(c);
    return rc;
}

int hb_ctx_epsl_step(hb_ctx *c, double vare, double veps_in, uint64_t seed, int64_t iter, double zJ, double chis, double s2_df)
{
    int rc = epsl_check(c, "hb_ctx_epsl_step");
    if (rc) return rc;
    hb_epsl *p = c->epsl;
    const int n = p->n, q = p->q, ne = p->ne;
    hipStream_t st = c->stream;
    // J (:555-564)
    hipLaunchKernelGGL(k_epsl_chunkdot, dim3(blocks(n)), dim3(ET), 0, st, p->yJ, c->r, n, p->parts);
    hipLaunchKernelGGL(k_epsl_jfin, dim3(1), dim3(ET), 0, st, p->parts, (int)blocks(n), p->st, p->JtJ, vare, zJ);
    hipLaunchKernelGGL(k_epsl_japply, dim3(blocks(n)), dim3(ET), 0, st, c->r, c->r32, c->u, p->yJ, n, p->st);
    // the pass (:565-570)
    hipLaunchKernelGGL(k_epsl_b, dim3(blocks(q)), dim3(ET), 0, st, c->r + p->tail0, p->rec_ptr, p->rec, p->zz, p->x, p->xold, p->b, q);
    HB_HIP(hipGetLastError());
    epsl_view v{};
    v.indptr = p->indptr;
    v.indices = p->indices;
    v.data = p->data;
    v.diag = p->diag;
    v.zz = p->zz;
    v.b = p->b;
    v.x = p->x;
    v.rows = p->rows;
    v.steps = p->steps;
    v.st = p->st;
    v.vare = vare;
    v.veps_in = veps_in;
    v.seed = seed;
    v.sub = hb_sub(HB_PURPOSE_EPSL, (uint64_t)iter);
    v.q = q;
    for (const hb_epsl_launch &l : p->plan.launches) {
        if (l.kind == 0) hipLaunchKernelGGL(k_epsl_narrow, dim3(1), dim3(ET), 0, st, v, l.s0, l.s1);
        else {
            const hb_epsl_step &e = p->plan.steps[l.s0];
            const int nb_lane = (e.nlane + ET - 1) / ET, nb_wave = (e.nwave + ET / 64 - 1) / (ET / 64);
            hipLaunchKernelGGL(k_epsl_wide, dim3((unsigned)(nb_lane + nb_wave)), dim3(ET), 0, st, v, l.s0, nb_lane);
        }
    }
    HB_HIP(hipGetLastError());
    // the residual (:572-576) and veps (:577-583)
    hipLaunchKernelGGL(k_epsl_scatter, dim3(blocks(ne)), dim3(ET), 0, st, c->r + p->tail0, c->r32 + p->tail0, c->u + p->tail0, p->idx, p->xold, p->x, ne);
    hipLaunchKernelGGL(k_epsl_gx, dim3(blocks(q)), dim3(ET), 0, st, p->indptr, p->indices, p->data, p->x, p->t, q);
    hipLaunchKernelGGL(k_epsl_chunkdot, dim3(blocks(q)), dim3(ET), 0, st, p->x, p->t, q, p->parts);
    hipLaunchKernelGGL(k_epsl_vfin, dim3(1), dim3(ET), 0, st, p->parts, (int)blocks(q), p->st, s2_df, chis);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hb_ctx_epsl_state(hb_ctx *c, double *x, double *veps, double *qv, double *J)
{
    int rc = epsl_check(c, "hb_ctx_epsl_state");
    if (rc) return rc;
    hb_epsl *p = c->epsl;
    rc = hb_epsl_fetch_enqueue(c);
    if (rc) return rc;
    if (x) HB_HIP(hipMemcpyAsync(x, p->x, sizeof(double) * (size_t)p->q, hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    if (veps) *veps = p->h_st[0];
    if (qv) *qv = p->h_st[1];
    if (J) *J = p->h_st[2];
    return HB_OK;
}

int hb_ctx_epsl_debug_get(hb_ctx *c, double *b, double *x_old, double *rhs, int32_t *counts)
{
    int rc = epsl_check(c, "hb_ctx_epsl_debug_get");
    if (rc) return rc;
    hb_epsl *p = c->epsl;
    HB_HIP(hipStreamSynchronize(c->stream));
    const size_t nb = sizeof(double) * (size_t)p->q;
    if (b) HB_HIP(hipMemcpy(b, p->b, nb, hipMemcpyDeviceToHost));
    if (x_old) HB_HIP(hipMemcpy(x_old, p->xold, nb, hipMemcpyDeviceToHost));
    if (rhs) HB_HIP(hipMemcpy(rhs, p->st + 3, sizeof(double), hipMemcpyDeviceToHost));
    if (counts) {
        counts[0] = (int32_t)p->plan.steps.size();
        counts[1] = (int32_t)p->plan.launches.size();
        counts[2] = p->plan.levels;
        counts[3] = p->plan.max_col;
    }
    return HB_OK;
}

int hb_ctx_epsl_debug_set(hb_ctx *c, int32_t sched_mode, int32_t row_mode)
{
    int rc = epsl_check(c, "hb_ctx_epsl_debug_set");
    if (rc) return rc;
    if (sched_mode < 0 || sched_mode > 2 || row_mode < 0 || row_mode > 2) return hb_fail(HB_ERR_INVALID, "hb_ctx_epsl_debug_set: modes are 0, 1 or 2");
    c->epsl->sched_mode = sched_mode;
    c->epsl->row_mode = row_mode;
    return epsl_plan_upload(c);
}

} // extern "C"
