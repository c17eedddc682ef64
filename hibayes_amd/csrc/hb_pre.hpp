// hb_pre.hpp — what a sweep computes per marker outside its chain, one text for the chain kernels' unit (hb_kernels.hip: k_pre,
// k_bayesl_post) and the sparse summary-level sampler's (hb_sbayes_sparse.hip: k_ss_pre, k_ss_bayesl_post): pre_marker — everything
// that does not depend on the running right-hand side (deviates, 1/v, sd*z, the inclusion test as thresholds on rhs^2) —, BayesL's
// variance draw, and the GWAS windows' kernel. Self-contained: either unit includes it.
#pragma once
#include "../../include/hibayes_gpu.h"
#include "hb_rng.hpp"
#include "hb_wave.hpp"

// ---------------------------------------------------------------------------------------------
// pre_marker: everything per marker that does not depend on the running rhs.
// Conditional posteriors restated as thresholds on q = rhs^2:
//   B/C (src/Bayes.cpp:640-645 / :683-688): included  <=>  U >= 1/(1+exp(s1-s0))
//        <=>  s1-s0 >= log((1-U)/U)  <=>  q >= 2 v vare (log((1-U)/U) + ldV/2 - logpi1 + logpi0)
//   R   (:759-781): class > c  <=>  U >= P(class <= c | q); with fold ascending that cumulative
//        probability decreases in q, so the K-1 boundaries are thresholds thr_0 <= thr_1 <= ...
//        found here by safeguarded Newton on  log B(q) - log A(q) = log((1-U)/U).
// ---------------------------------------------------------------------------------------------
// (static: a header that more than one unit includes defines nothing with external linkage)
static __device__ double bayesr_threshold(int K, int c, const double *a, const double *b, double logT)
{
    // h(q) = logsumexp_{i>c}(a_i + b_i q) - logsumexp_{i<=c}(a_i + b_i q) - logT, increasing in q
    // (exp(0) = 1 and log(1) = 0 exactly: the term that IS its group's maximum needs no exp, a one-term group no log — the
    // same numbers with about half of the transcendental calls; this function is most of k_pre's millisecond for BayesR)
    auto h = [&](double q, double &dh) {
        double mA = -HB_INF, mB = -HB_INF;
        for (int i = 0; i < K; i++) {
            const double s = a[i] + b[i] * q;
            if (i <= c) mA = fmax(mA, s); else mB = fmax(mB, s);
        }
        double sA = 0, sB = 0, dA = 0, dB = 0;
        for (int i = 0; i < K; i++) {
            const double s = a[i] + b[i] * q;
            if (i <= c) { const double w = s == mA ? 1.0 : exp(s - mA); sA += w; dA += b[i] * w; }
            else        { const double w = s == mB ? 1.0 : exp(s - mB); sB += w; dB += b[i] * w; }
        }
        dh = dB / sB - dA / sA;
        return (mB + (sB == 1.0 ? 0.0 : log(sB))) - (mA + (sA == 1.0 ? 0.0 : log(sA))) - logT;
    };
    double dh;
    double h0 = h(0.0, dh);
    if (!(h0 < 0.0)) return 0.0;         // already above the boundary at q = 0
    if (!(dh > 0.0)) return HB_INF;      // flat: the boundary is never crossed
    // bracket
    double lo = 0.0, hi = -h0 / dh;
    if (!(hi > 0.0)) hi = 1.0;
    double hh = h(hi, dh);
    int guard = 0;
    while (hh < 0.0 && guard++ < 200) {
        lo = hi;
        hi *= 2.0;
        hh = h(hi, dh);
    }
    if (hh < 0.0) return HB_INF;
    double q = hi;
    for (int it = 0; it < 100; it++) {
        double d;
        const double hv = h(q, d);
        if (hv < 0.0) lo = q; else hi = q;
        // Round 6: a Newton step below the last bits of q means q IS the root — stop. The test used to come only after the safeguard, and the
        // safeguard rejects a step of zero (qn == q == hi is not inside (lo, hi)): a search that had converged in four steps then bisected
        // its whole bracket again, fifty evaluations of four exp and two log each — one boundary in ten, i.e. nearly every wave: k_pre was
        // 1.09 ms of a BayesR sweep at m = 500 000 (a tenth of a converged sweep, nothing beside it) and is 0.2 now; at most eleven evaluations
        // instead of sixty-two, the same roots to 2e-13 (measured offline over 18 000 boundaries, tools/r6_newton_sim.py).
        const double step = hv / d;
        if (fabs(step) <= 4e-16 * fabs(q)) break;
        double qn = q - step;
        if (!(qn > lo && qn < hi)) qn = 0.5 * (lo + hi);
        if (fabs(qn - q) <= 4e-16 * fabs(qn) || hi - lo <= 4e-16 * hi) { q = qn; break; }
        q = qn;
    }
    return q;
}

// does marker j of the view take part: inside the marker set, with statistics (the others get thresholds that nobody crosses)
template <class View>
__device__ __forceinline__ bool pre_active(const View &v, int j) { return (j < v.m) && (v.vx[j] != 0.0); }

// One marker's coefficients. v: the caller's view (hb_kernels.hip's pre_view, hb_sbayes_sparse.hip's ss_view: the members used
// below); vare: the residual variance the marker is sampled under; marker: its index in the whole marker set, which addresses its
// random streams. SS: the summary-level sampler's rule for BayesB / BayesC — its chain can draw a negative or NaN variance, so the
// threshold carries a sign in v.sgn[j] (which the caller has set to +1; ss_included, hb_sbayes_sparse.hip) and a NaN s1 includes
// the marker. Source lines: src/Bayes.cpp's (what k_pre and the dense summary-level sampler follow), then "S" src/SBayesS.cpp's.
template <bool SS, class View>
__device__ __forceinline__ void pre_marker(const hb_sweep_in *__restrict__ pin, const View &v, int j, double vare, int64_t marker)
{
    const int kp = v.kpad;
    if (!pre_active(v, j)) {
        for (int c = 0; c < kp; c++) {
            v.thr[(int64_t)c * v.m_pad + j] = HB_INF;
            v.invv[(int64_t)c * v.m_pad + j] = 0.0;
            v.sdz[(int64_t)c * v.m_pad + j] = 0.0;
        }
        return;
    }
    const int model = pin->model_index;
    const uint64_t sub = hb_sub(HB_PURPOSE_MARKER, (uint64_t)pin->iter);
    const uint64_t base = (uint64_t)marker * HB_BLK_PER_MARKER;
    const double xx = v.xpx[j];
    const double gold = v.g[j];
    const double z = hb_normal_blk(v.seed, sub, base + 1);

    if (model == 6) {
        const int K = pin->n_fold;
        const double U = hb_uniform_blk(v.seed, sub, base + 0);
        const double logT = log((1.0 - U) / U);
        double a[HB_MAX_FOLD], b[HB_MAX_FOLD];
        a[0] = pin->logpi[0];
        b[0] = 0.0;
        const double lhs = xx / vare;
        for (int c = 1; c < K; c++) {
            const double vf = pin->vara_fold[c];
            const double vv = xx + vare / vf; // :761, :784; S :462, :487
            a[c] = -0.5 * log(vf * lhs + 1.0) + pin->logpi[c];
            b[c] = 0.5 / (vv * vare);
            v.invv[(int64_t)(c - 1) * v.m_pad + j] = 1.0 / vv;
            v.sdz[(int64_t)(c - 1) * v.m_pad + j] = sqrt(vare / vv) * z;
        }
        double prev = 0.0;
        for (int c = 0; c < K - 1; c++) { // boundaries are nested: thr_0 <= thr_1 <= ...
            prev = fmax(prev, bayesr_threshold(K, c, a, b, logT));
            v.thr[(int64_t)c * v.m_pad + j] = prev;
        }
        for (int c = K - 1; c < kp; c++) {
            v.thr[(int64_t)c * v.m_pad + j] = HB_INF;
            v.invv[(int64_t)c * v.m_pad + j] = 0.0;
            v.sdz[(int64_t)c * v.m_pad + j] = 0.0;
        }
        return;
    }

    double varg = pin->varg;
    if (model == 2 || model == 3) { // per-marker variance, :613 / :636; S :308 / :332 — drawn from g of the previous sweep
        hb_stream st(v.seed, sub, base + 4);
        varg = (gold * gold + pin->s2varg_df) / st.chisq(pin->dfvara + 1.0);
    }
    double vv;
    if (model == 5) vv = xx + 1.0 / v.vargL[j]; // :726; S :427 (and sqrt(varei / v), S :428)
    else vv = xx + vare / varg;                 // :595, :617, :648, :691; S :289, :313, :346, :386
    double thr = -HB_INF;
    if (model == 3 || model == 4) {
        const double U = hb_uniform_blk(v.seed, sub, base + 0);
        if constexpr (!SS) {
            const double logdetV = log(varg * (xx / vare) + 1.0);
            thr = 2.0 * vv * vare * (log((1.0 - U) / U) + 0.5 * logdetV - pin->logpi[1] + pin->logpi[0]);
            if (thr != thr) thr = HB_INF; // inf - inf when both log(pi) are -inf: never include
        } else {
            const double logdetV = log(varg * (xx / vare) + 1.0), w = 2.0 * vv * vare;
            if (logdetV != logdetV || w != w) {
                thr = -HB_INF; // s1 is NaN (a negative or NaN variance): `uniform < acceptProb` is false, the marker is in (S :380-383)
            } else {
                thr = w * (log((1.0 - U) / U) + 0.5 * logdetV - pin->logpi[1] + pin->logpi[0]);
                if (thr != thr) thr = HB_INF; // inf - inf when both log(pi) are -inf: never include
                else if (w < 0.0) v.sgn[j] = -1.0;
            }
        }
    }
    v.thr[j] = thr;
    v.invv[j] = 1.0 / vv;
    v.sdz[j] = sqrt(vare / vv) * z;
    for (int c = 1; c < kp; c++) {
        v.thr[(int64_t)c * v.m_pad + j] = HB_INF;
        v.invv[(int64_t)c * v.m_pad + j] = 0.0;
        v.sdz[(int64_t)c * v.m_pad + j] = 0.0;
    }
}

// BayesL: vargL_j <- 1 / InvGauss(sqrt(vare) lambda / |g_j|, lambda^2) from the marker's own stream (order-free); `strict` keeps a
// draw > 0, otherwise >= 0 (the callers cite their references' lines)
__device__ __forceinline__ void bayesl_post_marker(const hb_sweep_in *__restrict__ pin, uint64_t seed, int64_t marker, double vare, double g,
                                                   double *__restrict__ vargL, int strict)
{
    const uint64_t sub = hb_sub(HB_PURPOSE_MARKER, (uint64_t)pin->iter);
    hb_stream st(seed, sub, (uint64_t)marker * HB_BLK_PER_MARKER + 2);
    const double vargi = 1.0 / st.invgauss(sqrt(vare) * pin->lambda / fabs(g), pin->lambda2);
    if (strict ? vargi > 0.0 : vargi >= 0.0) *vargL = vargi;
}

// GWAS windows: a window flagged in this sweep counts once (static: each unit that includes this header has its own)
static __global__ void k_windows(uint8_t *__restrict__ wflag, double *__restrict__ wppa, int nw)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    wppa[w] += (double)wflag[w];
    wflag[w] = 0;
}
