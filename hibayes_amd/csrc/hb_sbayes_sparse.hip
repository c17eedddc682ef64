// hb_sbayes_sparse.hip — device side of the summary-level sampler on a SPARSE LD matrix: SBayesS() of the reference
// (src/SBayesS.cpp:277-600) from the handle's device CSC (hb_ldm_device_csc: int64 column pointers, int32 rows sorted inside a
// column, fp64 values). The host loop is hb_sbayes.hip (hb_sbayes_run_sparse). A unit of its own, so that the chain kernels' unit gains
// no instantiation; what it shares with hb_kernels.hip it includes: the per-marker coefficients, BayesL's draw and the windows' kernel
// (hb_pre.hpp), the wave and block sums (hb_wave.hpp). k_ss_group keeps its own text of k_sb_group's round scaffolding (hb_sbayes.hpp
// says why).
//
// SBayesS() is not SBayesD() with zeros: marker i is sampled under its own residual variance varei = varediff[i] vara + vare
// (:285), BayesC / BayesCpi / BayesR effects with g^2 vx > vary are redrawn, at most 101 times (:388-398, :489-499), and a move
// walks the stored entries of its column (:292-296). The matrix is symmetric (hb_ldm_from_csc checks it, hb_ldm_build's are by
// construction), so row j of the matrix is column j of the CSC: every fold below is a PULL — the owner of a row walks its own
// column and adds the moved markers' terms in marker order, the order of the reference's daxpy sequence. There is no
// floating-point atomic and no sum whose order the hardware chooses: two runs of one call agree bit for bit.
//
// A sweep runs in groups of SS_GS = 512 consecutive markers, like hb_sbayes.hpp's, two kernels per group:
//   k_ss_group   ONE workgroup, thread = marker of the group, k_sb_group's scheme: rounds of up to 64 candidates in marker order;
//                their mutual LD entries scattered from each candidate's column run inside the group's rows (contiguous, found
//                once when the CSC is made) through an LDS table "position in group -> candidate rank"; the exact serial chain
//                on wave 0; the round's moves pulled onto the later markers of the group through an LDS table of n (g_old - g_new)
//                by position; a marker the round passed over that is pushed over its threshold joins and the round is repeated.
//   k_ss_update  r_hat[j] += sum over the group's moves of n (g_old - g_new)_k ldm[j][k] for the rows [row_lo, row_hi) the
//                group's columns touch (fixed when the CSC is made: it sizes the grid), thread = row; a row keeps its place
//                in its column from group to group (the groups come in ascending order), so a sweep reads every entry once.
// One sweep = 2 ceil(m / 512) + 3 launches (+ 1 for BayesL), captured once and replayed.
#include "hb_sbayes_sparse.hpp"
#include "hb_plan.hpp"
#include "hb_pre.hpp"

namespace {

// The inclusion test on q = rhs^2. pre_marker's threshold form "q >= thr" comes from multiplying s1 - s0 >= log((1 - U) / U) by
// 2 v varei, which the reference's own chain can make NEGATIVE: on an indefinite (thresholded) matrix g' ldm g, and with it the
// sweep's Vg and then Ve, can be drawn below zero (src/SBayesS.cpp:531, :538). The reference goes on — the inequality turns round
// (sg < 0: included <=> q <= thr), and where log(varg lhs + 1), sqrt(varei / v) or the right-hand side itself is NaN,
// `uniform < acceptProb` is false and the marker is INCLUDED with a NaN effect (:380-387). The same here: a NaN q is in.
__device__ __forceinline__ bool ss_included(double q, double thr, double sg) { return sg >= 0.0 ? !(q < thr) : !(q > thr); }

struct ss_view {
    int m, m_pad, n;
    uint64_t seed;
    const int64_t *cp, *run;
    const int32_t *ri, *runn;
    const double *va;
    double *r_hat;
    const double *xy;
    double *g;
    const double *xpx, *vx, *vxt; // vx[i] != 0 <=> marker i has summary statistics; vxt[i] = ldm[i][i]
    const double *varediff;
    double *varei, *vargL;
    double *thr, *invv, *sdz;
    double *sgn;      // +1, or -1 where the marker's 2 v varei is negative this sweep (ss_included)
    const double *ex; // vara, vary
    uint8_t *tracker;
    uint32_t *nzrate;
    int *ev_n;
    double *gtab, *rd;
    int32_t *cursor;
    const uint32_t *wind;
    uint8_t *wflag;
    double *acc;
    int kpad;
};

// pre_marker with the marker's own varei = varediff[i] vara + vare (src/SBayesS.cpp:285) where k_pre has vare; also the sweep's start:
// every row's place in its column back to 0, no marker redrawn yet, every sign +1
__global__ __launch_bounds__(256) void k_ss_pre(const hb_sweep_in *__restrict__ pin, ss_view v)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= v.m_pad) return;
    if (j == 0) {
        v.rd[0] = -1.0;
        v.rd[1] = 0.0;
    }
    v.cursor[j] = 0;
    v.sgn[j] = 1.0;
    const double vare = pre_active(v, j) ? v.varediff[j] * v.ex[0] + pin->vare : 0.0;
    v.varei[j] = vare;
    pre_marker<true>(pin, v, j, vare, j);
}

// BayesL: vargL_j <- 1 / InvGauss(sqrt(varei_j) lambda / |g_j|, lambda^2), kept when > 0 (:430-431)
__global__ __launch_bounds__(256) void k_ss_bayesl_post(const hb_sweep_in *__restrict__ pin, ss_view v)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= v.m || v.vx[j] == 0.0) return;
    bayesl_post_marker(pin, v.seed, j, v.varei[j], v.g[j], &v.vargL[j], 1);
}

template <int K1>
__global__ __launch_bounds__(SS_GS) void k_ss_group(const hb_sweep_in *__restrict__ pin, ss_view v, int g0)
{
    __shared__ double cs_d[(5 + 3 * K1) * 64]; // the round's candidates by rank: rhs, g_old, varei, vx, sign, thr[K1], 1/v [K1], sd z [K1]
    __shared__ double cg[64 * 64];             // cg[k][c] = ldm[c][k] for k < c (candidate ranks), zero elsewhere
    __shared__ double dtab[SS_GS];             // n (g_old - g_new) of the round's moves by position in the group, zero elsewhere
    __shared__ double res_g[64], red[SS_GS / 64];
    __shared__ long long cs_run[64];
    __shared__ int p2r[SS_GS];                 // position in group -> candidate rank of the round, -1: not a candidate
    __shared__ int cs_pos[64], cs_runn[64], res_c[64], wcnt[SS_GS / 64], misc[4];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, i = g0 + t;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const bool in = i < v.m;
    const int ic = min(i, v.m - 1); // (loads of a thread past the end go to an address that exists)
    const int model = pin->model_index;
    const bool trunc = model == 4 || model == 6;
    const double vary = v.ex[1];
    const uint64_t subr = hb_sub(HB_PURPOSE_REDRAW, (uint64_t)pin->iter);
    const double vxi = v.vx[ic], gi0 = v.g[ic], xx = v.xpx[ic], vei = v.varei[ic], vxt = v.vxt[ic], sg = v.sgn[ic];
    const long long run0 = v.run[ic];
    const int runn = in ? v.runn[ic] : 0;
    double thr[K1], invv[K1], sdz[K1];
#pragma unroll
    for (int c = 0; c < K1; c++) {
        thr[c] = v.thr[(size_t)c * v.m_pad + ic];
        invv[c] = v.invv[(size_t)c * v.m_pad + ic];
        sdz[c] = v.sdz[(size_t)c * v.m_pad + ic];
    }
    double r0 = v.r_hat[ic]; // the marker's right-hand side with every move BEFORE the current round applied (without xx g_old)
    const bool active = in && vxi != 0.0;
    const double gold = in ? gi0 : 0.0;
#pragma unroll
    for (int c = 0; c < K1; c++) thr[c] = active ? thr[c] : HB_INF;
    const int gend = min(SS_GS, v.m - g0);
    const double nn = (double)v.n;
    int pos_lo = 0, nev_total = 0;
    bool forced = false, decided = false;
    int my_cls = 0;
    double my_gn = 0.0;
    for (;;) {
        // ---- the round's candidates, ranked in marker order ----
        const bool isc = active && t >= pos_lo && (gold != 0.0 || forced || ss_included(r0 * r0, thr[0], sg));
        const unsigned long long cm = __ballot(isc);
        if (lane == 0) wcnt[wave] = __popcll(cm);
        if (t == 0) misc[1] = gend;
        __syncthreads(); // B1
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < SS_GS / 64; w++) {
            const int c = wcnt[w];
            before += (w < wave) ? c : 0;
            total += c;
        }
        if (total == 0) break; // nobody (left) in the group can move
        const int rank = before + __popcll(cm & lt), ncr = min(total, 64);
        const bool mine = isc && rank < 64;
        if (isc && rank == 64) misc[1] = t; // the round ends before the 65th candidate
        if (mine) {
            cs_d[rank] = (gold != 0.0) ? fma(xx, gold, r0) : r0; // :286-287: rhs = r_hat[i] (+ xx g when g != 0)
            cs_d[64 + rank] = gold;
            cs_d[128 + rank] = vei;
            cs_d[192 + rank] = vxt;
            cs_d[256 + rank] = sg;
#pragma unroll
            for (int c = 0; c < K1; c++) {
                cs_d[(5 + c) * 64 + rank] = thr[c];
                cs_d[(5 + K1 + c) * 64 + rank] = invv[c];
                cs_d[(5 + 2 * K1 + c) * 64 + rank] = sdz[c];
            }
            cs_pos[rank] = t;
            cs_run[rank] = run0;
            cs_runn[rank] = runn;
        }
        p2r[t] = mine ? rank : -1;
        dtab[t] = 0.0;
#pragma unroll
        for (int u = 0; u < 8; u++) cg[u * SS_GS + t] = 0.0;
        __syncthreads(); // B2
        const int pos_hi = misc[1];
        // ---- LD entries among the round's candidates: a wave walks candidate c's column inside the group's rows; the entry
        //      in the row of an earlier candidate k is ldm[k][c] = ldm[c][k] ----
        for (int c = wave; c < ncr; c += SS_GS / 64) {
            const long long lo = cs_run[c];
            const int ne = cs_runn[c];
            for (int e = lane; e < ne; e += 64) {
                const int k = p2r[v.ri[lo + e] - g0];
                if (k >= 0 && k < c) cg[k * 64 + c] = v.va[lo + e];
            }
        }
        __syncthreads(); // B3
        // ---- the exact serial chain over the round's candidates: wave 0, one candidate per lane, in marker order ----
        bool redrew = false;
        double last2 = 0.0;
        int cp = 0;
        if (wave == 0) {
            const bool lv = lane < ncr;
            double crhs = lv ? cs_d[lane] : 0.0;
            const double cgold = lv ? cs_d[64 + lane] : 0.0, cvei = lv ? cs_d[128 + lane] : 0.0, cvx = lv ? cs_d[192 + lane] : 0.0;
            const double csg = lv ? cs_d[256 + lane] : 1.0;
            double cthr[K1], cinvv[K1], csdz[K1];
#pragma unroll
            for (int c = 0; c < K1; c++) {
                cthr[c] = lv ? cs_d[(5 + c) * 64 + lane] : HB_INF;
                cinvv[c] = lv ? cs_d[(5 + K1 + c) * 64 + lane] : 0.0;
                csdz[c] = lv ? cs_d[(5 + 2 * K1 + c) * 64 + lane] : 0.0;
            }
            cp = lv ? cs_pos[lane] : 0;
            const uint64_t rblk = (uint64_t)(g0 + cp) * SS_REDRAW_BLK;
            // `fin`: this lane's right-hand side is final, the value is the marker's draw — only then is the truncation's loop run
            auto decide = [&](double rhsv, bool fin, int &cls, double &gn) {
                const double q = rhsv * rhsv;
                double gsel = fma(rhsv, cinvv[0], csdz[0]), isel = cinvv[0];
                const bool inc = ss_included(q, cthr[0], csg);
                cls = inc ? 1 : 0;
#pragma unroll
                for (int c = 1; c < K1; c++) {
                    const bool ge = q >= cthr[c];
                    cls += ge ? 1 : 0;
                    gsel = ge ? fma(rhsv, cinvv[c], csdz[c]) : gsel;
                    isel = ge ? cinvv[c] : isel;
                }
                gn = inc ? gsel : 0.0;
                if (K1 == 1 && model == 5 && fabs(gn) < 1e-6) gn = 1e-6; // :429
                if (trunc && fin && cls > 0 && gn * gn * cvx > vary) {    // :388-398 / :489-499 (cold: sd is recomputed)
                    const double sd = sqrt(cvei * isel);
                    int ii = 0;
                    do {
                        ii++;
                        gn = fma(sd, hb_normal_blk(v.seed, subr, rblk + (uint64_t)ii), rhsv * isel);
                        last2 = gn * gn; // :392 vargi = gi * gi
                        if (ii > 100) gn = 0.0;
                    } while (gn * gn * cvx > vary);
                    redrew = true;
                }
            };
            double rnext = cg[lane]; // row k of cg, one step ahead
            for (int k = 0; k < ncr; k++) {
                const double rcur = rnext;
                rnext = cg[min(k + 1, ncr - 1) * 64 + lane];
                int cls;
                double gn;
                decide(crhs, lane == k, cls, gn);
                const double gk = readlane_f64((cgold - gn) * nn, k); // :291 gi_ = (g[i] - gi) * n
                if (rcur != 0.0) crhs = fma(gk, rcur, crhs); // r_hat[lane] += gi_ ldm[lane][k], at the stored rows of column k only (row k of cg is zero at and before lane k; a NaN gi_ must not reach a row the column does not store)
            }
            int cls;
            double gn;
            redrew = false;
            decide(crhs, lv, cls, gn); // lane k's rhs was not touched after its own step
            const double gi_ = lv ? (cgold - gn) * nn : 0.0;
            const unsigned long long moved = __ballot(gi_ != 0.0);
            if (gi_ != 0.0) dtab[cp] = gi_;
            res_c[lane] = cls;
            res_g[lane] = gn;
            if (lane == 0) misc[0] = __popcll(moved);
        }
        __syncthreads(); // B4
        const int nmoves = misc[0];
        // ---- the round's moves onto the later markers of the group: the thread walks its own column inside the group's rows
        //      (= its row, by symmetry) up to itself, the moved markers' terms in marker order ----
        double rnew = r0;
        if (nmoves)
            for (int e = 0; e < runn; e++) {
                const int p = v.ri[run0 + e] - g0;
                if (p >= t) break;
                const double dl = dtab[p];
                if (dl != 0.0) rnew = fma(dl, v.va[run0 + e], rnew);
            }
        // ---- did every marker the round passed over really stay below its threshold? ----
        const bool viol = active && !isc && t >= pos_lo && t < pos_hi && ss_included(rnew * rnew, thr[0], sg);
        if (__syncthreads_or(viol ? 1 : 0)) { // B5: roll the round back, the markers that crossed join the candidates
            forced = forced || viol;
            continue;
        }
        // ---- commit the round ----
        r0 = rnew;
        if (mine) {
            decided = true;
            my_cls = res_c[rank];
            my_gn = res_g[rank];
        }
        if (wave == 0) { // the sweep's last redrawn marker so far (rounds and groups come in marker order)
            const unsigned long long rm = __ballot(redrew);
            if (rm != 0ull && lane == 63 - __clzll((long long)rm)) {
                v.rd[0] = (double)(g0 + cp);
                v.rd[1] = last2;
            }
        }
        nev_total += nmoves;
        pos_lo = pos_hi;
        if (pos_lo >= gend) break;
    }
    // ---- the group's outcome ----
    if (!active || !decided) { my_cls = 0; my_gn = 0.0; }
    if (in) {
        if (my_gn != gold) v.g[i] = my_gn;
        v.tracker[i] = (uint8_t)my_cls;
        if (pin->count_pip && my_cls != 0) {
            v.nzrate[i] += 1u;
            if (v.wind) v.wflag[v.wind[i] - 1u] = 1;
        }
    }
    v.gtab[t] = in ? (gold - my_gn) * nn : 0.0; // k_ss_update's table: a marker moves at most once per sweep
    if (t == 0) *v.ev_n = nev_total;
    // class counts (sum g^2 is formed at the end of the sweep, k_ss_reduce: it depends on the sweep's last redraw)
#pragma unroll
    for (int c = 0; c <= K1; c++) {
        const double cnt = block_sum((active && my_cls == c) ? 1.0 : 0.0, red);
        if (t == 0 && cnt != 0.0 && c < HB_MAX_FOLD) v.acc[HB_ACC_COUNT0 + c] += cnt; // (one chain kernel at a time: no atomics needed)
    }
    if (t == 0) v.acc[HB_ACC_EVENTS] += (double)nev_total;
}

// r_hat[j] += sum over the group's moved markers k of n (g_old - g_new)_k ldm[j][k], rows [row_lo, row_hi); thread = row j, which
// walks column j (= row j) over the group's rows from where the previous group left it
__global__ __launch_bounds__(256) void k_ss_update(ss_view v, int g0, int row_lo, int row_hi)
{
    __shared__ double s_tab[SS_GS];
    if (*v.ev_n == 0) return; // (uniform)
    for (int k = threadIdx.x; k < SS_GS; k += 256) s_tab[k] = v.gtab[k];
    __syncthreads();
    const int j = row_lo + blockIdx.x * 256 + threadIdx.x;
    if (j >= row_hi) return;
    const int g1 = min(g0 + SS_GS, v.m);
    const int64_t end = v.cp[j + 1];
    int64_t e = v.cp[j] + v.cursor[j];
    while (e < end && v.ri[e] < g0) e++;
    double a = v.r_hat[j];
    bool any = false;
    for (; e < end; e++) {
        const int r = v.ri[e];
        if (r >= g1) break;
        const double dl = s_tab[r - g0];
        if (dl != 0.0) {
            a = fma(dl, v.va[e], a); // in marker order, as the reference's daxpy sequence
            any = true;
        }
    }
    v.cursor[j] = (int32_t)(e - v.cp[j]);
    if (any) v.r_hat[j] = a;
}

// end of sweep: g . (xy - r_hat) and g . (xy + r_hat) (:529-537), sum of vargL (BayesL :443), and the sweep's sum of squared
// effects: g . g (RR :299), the sum over the included of g^2 / fold[class] (R :500) or of g^2 (C :399) — in C from the last
// redrawn marker on, plus its last draw squared (`vargi = gi * gi` inside the loop, :392, starts the sum again). One workgroup.
__global__ __launch_bounds__(1024) void k_ss_reduce(const hb_sweep_in *__restrict__ pin, ss_view v, int want_vargl)
{
    __shared__ double red[16];
    const int model = pin->model_index;
    const int first = (model == 4 && v.rd[0] >= 0.0) ? (int)v.rd[0] : 0;
    double s1 = 0, s2 = 0, s3 = 0, s4 = 0;
    for (int i = threadIdx.x; i < v.m; i += blockDim.x) {
        const double gi = v.g[i], x = v.xy[i], r = v.r_hat[i];
        s1 = fma(gi, x - r, s1);
        s2 = fma(gi, x + r, s2);
        if (want_vargl) s3 += v.vargL[i];
        const int cls = v.tracker[i];
        if (cls > 0 && i >= first) s4 += (model == 6) ? gi * gi / pin->fold[cls] : gi * gi;
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    s3 = block_sum(s3, red);
    s4 = block_sum(s4, red);
    if (threadIdx.x == 0) {
        v.acc[HB_ACC_SUMR] = s1;
        v.acc[HB_ACC_SUMR2] = s2;
        v.acc[HB_ACC_SUMVARGL] = s3;
        v.acc[HB_ACC_SUMG2] = (model == 4 && v.rd[0] >= 0.0) ? v.rd[1] + s4 : s4;
    }
}

__global__ void k_ss_varediff(const int32_t *__restrict__ cnt, int m, double *__restrict__ out)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m) out[j] = ((double)m - (double)cnt[j]) / (double)m; // :140
}

} // namespace

// ---- launchers (hb_sbayes.hip owns the buffers: struct hb_ss_dev) ----
int hbk_ss_enqueue_sweep(hb_ss_dev *s, int model, int n_fold)
{
    hb_sb_dev *d = &s->b;
    const int kp = kpad_for(model, n_fold);
    ss_view v{d->m, d->m_pad, d->n, d->seed, s->csc.cp, s->csc.run, s->csc.ri, s->csc.runn, s->csc.va, d->r_hat, d->xy, d->g, d->xpx,
              d->vx, s->vxt, s->varediff, s->varei, d->vargL, d->thr, d->invv, d->sdz, s->sgn, s->ex, d->tracker, d->nzrate, d->ev_n, s->gtab,
              s->rd, s->cursor, d->wind, d->wflag, d->acc, kp};
    HB_HIP(hipMemsetAsync(d->acc, 0, sizeof(double) * HB_ACC_N, d->stream));
    hipLaunchKernelGGL(k_ss_pre, dim3((d->m_pad + 255) / 256), dim3(256), 0, d->stream, d->d_in, v);
    for (int g0 = 0, gi = 0; g0 < d->m; g0 += SS_GS, gi++) {
        if (kp == 1) hipLaunchKernelGGL(k_ss_group<1>, dim3(1), dim3(SS_GS), 0, d->stream, d->d_in, v, g0);
        else if (kp == 3) hipLaunchKernelGGL(k_ss_group<3>, dim3(1), dim3(SS_GS), 0, d->stream, d->d_in, v, g0);
        else hipLaunchKernelGGL(k_ss_group<7>, dim3(1), dim3(SS_GS), 0, d->stream, d->d_in, v, g0);
        const int lo = s->csc.grp_lo[gi], hi = s->csc.grp_hi[gi];
        if (hi > lo) hipLaunchKernelGGL(k_ss_update, dim3((hi - lo + 255) / 256), dim3(256), 0, d->stream, v, g0, lo, hi);
    }
    if (model == 5) hipLaunchKernelGGL(k_ss_bayesl_post, dim3((d->m + 255) / 256), dim3(256), 0, d->stream, d->d_in, v);
    hipLaunchKernelGGL(k_ss_reduce, dim3(1), dim3(1024), 0, d->stream, d->d_in, v, model == 5 ? 1 : 0);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_ss_windows(hb_ss_dev *s)
{
    hb_sb_dev *d = &s->b;
    if (d->nw) hipLaunchKernelGGL(k_windows, dim3((d->nw + 255) / 256), dim3(256), 0, d->stream, d->wflag, d->wppa, d->nw);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_ss_varediff(hb_ss_dev *s)
{
    hb_sb_dev *d = &s->b;
    hipLaunchKernelGGL(k_ss_varediff, dim3((d->m + 255) / 256), dim3(256), 0, d->stream, s->csc.cnt, d->m, s->varediff);
    HB_HIP(hipGetLastError());
    return HB_OK;
}
