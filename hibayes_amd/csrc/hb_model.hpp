// hb_model.hpp — the model layer that Bayes() and SBayesD() / SBayesS() of the reference share line for line, once: the model's
// index, the checks of `Pi` and `fold` with the reference's texts, BayesR's class order, the prior defaults, a sweep's parameters from
// the chain's state, the hyper-parameter draws after a sweep, the progress line, the PIP rule and the summary statistics' population size. Plain C++ with nothing from HIP, so that it is tested on the CPU
// (tests/test_model_host.py). A refusal comes back as a status with its text in `err`; the callers hand both to hb_fail.
// hb_run.hip (individual level) and hb_sbayes.hip (summary level) interleave the three mixture checks with their other checks in
// different orders — each calls them where it made these checks before, so an input with several faults reports the same one.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>
#include "../../include/hibayes_gpu.h"
#include "hb_armasum.hpp"

static inline int hb_refuse(std::string &err, int status, const char *text)
{
    err = text;
    return status;
}

// (any other name, "BSLMM" among them, is 6 here: hb_run.hip maps that name to 4 itself)
static inline int hb_model_index(const std::string &model)
{
    return model == "BayesRR" ? 1 : model == "BayesA" ? 2 : (model == "BayesB" || model == "BayesBpi") ? 3
         : (model == "BayesC" || model == "BayesCpi") ? 4 : model == "BayesL" ? 5 : 6;
}

// 1. `Pi` and `fold` as given (src/Bayes.cpp:92-117, src/SBayesD.cpp:36-57): copies in Pi / fold, two zeros for a model without `fold`
static inline int hb_mixture_take(const std::string &model, const double *Pi_in, int n_pi, const double *fold_in, int n_fold_in,
                                  std::vector<double> &Pi, std::vector<double> &fold, std::string &err)
{
    if (n_pi < 2 || !Pi_in) return hb_refuse(err, HB_ERR_INVALID, "Pi should be a vector.");
    if (n_pi > HB_MAX_FOLD) return hb_refuse(err, HB_ERR_UNSUPPORTED, "more mixture classes than HB_MAX_FOLD");
    Pi.assign(Pi_in, Pi_in + n_pi);
    if (arma_sum(Pi.data(), Pi.size()) != 1) return hb_refuse(err, HB_ERR_INVALID, "sum of Pi should be 1.");
    if (Pi[0] == 1) return hb_refuse(err, HB_ERR_INVALID, "all markers have no effect size.");
    for (double p : Pi)
        if (p < 0 || p > 1) return hb_refuse(err, HB_ERR_INVALID, "elements of Pi should be at the range of [0, 1]");
    if (fold_in) {
        if (n_fold_in != n_pi) return hb_refuse(err, HB_ERR_INVALID, "length of Pi and fold not equals.");
        fold.assign(fold_in, fold_in + n_pi);
    } else {
        if (model == "BayesR") return hb_refuse(err, HB_ERR_INVALID, "'fold' should be provided for BayesR model.");
        if (n_pi != 2) return hb_refuse(err, HB_ERR_INVALID, "length of Pi and fold not equals.");
        fold.assign(2, 0.0);
    }
    return HB_OK;
}

// 2. the models that keep every marker in (src/Bayes.cpp:288-296): Pi = {0, 1} and fixed; the point-mass models other than BayesR
// take two classes
static inline int hb_mixture_always_in(const std::string &model, int model_index, std::vector<double> &Pi, bool &fixpi, bool &always_in,
                                       std::string &err)
{
    fixpi = (model == "BayesB" || model == "BayesC");
    always_in = (model_index == 1 || model_index == 2 || model_index == 5);
    if (always_in) {
        Pi[0] = 0;
        Pi[1] = 1;
        fixpi = true;
    } else if (model != "BayesR" && Pi.size() != 2) {
        return hb_refuse(err, HB_ERR_INVALID, "length of Pi should be 2, the first value is the proportion of non-effect markers.");
    }
    return HB_OK;
}

// 3. BayesR: the device evaluates the class boundaries as nested thresholds on q = rhs^2, which needs the non-null classes in
// order of increasing variance (P(class <= c | q) is then decreasing in q for every c). The reference takes `fold` in any
// order (src/Bayes.cpp:743-815) and walks the classes as given (:773-781) — with another order the same uniform picks another
// class, so no formulation can be that walk draw for draw AND monotone. The run is therefore the reference's chain for the
// classes SORTED by fold (the same posterior: the mixture does not depend on how its components are numbered); cls_of[]
// maps the internal class index back to the caller's for everything reported: pi, MCMCsamples$pi, the progress line.
static inline int hb_mixture_order(int model_index, std::vector<double> &Pi, std::vector<double> &fold, std::vector<int> &cls_of,
                                   std::string &err)
{
    const int n_fold = (int)fold.size();
    cls_of.resize(n_fold);
    for (int k = 0; k < n_fold; k++) cls_of[k] = k;
    if (model_index != 6) return HB_OK;
    std::stable_sort(cls_of.begin() + 1, cls_of.end(), [&](int x, int z) { return fold[x] < fold[z]; }); // class 0 is the null class (:759)
    std::vector<double> f2(n_fold), p2(n_fold);
    for (int k = 0; k < n_fold; k++) { f2[k] = fold[cls_of[k]]; p2[k] = Pi[cls_of[k]]; }
    fold = f2;
    Pi = p2;
    for (int k = 2; k < n_fold; k++)
        if (!(fold[k] > fold[k - 1]))
            return hb_refuse(err, HB_ERR_UNSUPPORTED, "BayesR on the GPU path needs distinct 'fold' values for the non-null classes");
    return HB_OK;
}

// ---- the hyper-parameter draws after a sweep: src/Bayes.cpp:603, :666-669, :710-716, :738-741, :803-814 and, the same lines,
// src/SBayesD.cpp:269, :321-324, :360-365, :386-389, :448-460 ----
struct hb_hyper_prior { // what a run fixes
    int model_index, n_fold;
    bool fixpi;
    double dfvara, s2varg, shape0, rate0;
    const double *fold;
};
struct hb_hyper_sums { // what one sweep leaves
    double sum_g2, sum_vargL;
    const double *class_count; // markers per class among the sampled ones (class 0 without the markers left out)
    // sampled markers n_used = n_total - nvar0, in the two terms of the reference's `dfvara_ + m - nvar0` and `shape0 + m - nvar0`:
    // (x + n_total) - nvar0 can differ from x + n_used in the last bit, and the draw would differ with it. The summary level
    // counts the sampled markers itself (count_y) and passes nvar0 = 0.
    double n_total, nvar0;
};
struct hb_hyper_state { // the chain's hyper-parameters, updated in place; the arrays have n_fold entries
    double &varg, &lambda, &lambda2;
    long long &NnzSnp;
    double *Pi, *vara_fold, *fold_snp_num;
};

// Stream: gamma(shape, scale) and chisq(df) (hb_stream of hb_rng.hpp; a recording fake in the test). The calls, their arguments
// and their order are the reference's.
template <class Stream> static inline void hb_draw_hyper(Stream &hs, const hb_hyper_prior &p, const hb_hyper_sums &s, hb_hyper_state st)
{
    auto draw_pi = [&]() { // rdirichlet_sample, src/stats.cpp:69-76
        std::vector<double> xn(p.n_fold);
        for (int j = 0; j < p.n_fold; j++) xn[j] = hs.gamma(st.fold_snp_num[j] + 1, 1.0);
        const double sx = arma_sum(xn.data(), xn.size());
        for (int j = 0; j < p.n_fold; j++) st.Pi[j] = xn[j] / sx;
    };
    switch (p.model_index) {
    case 1: // :603
        st.varg = (s.sum_g2 + p.s2varg * p.dfvara) / hs.chisq(p.dfvara + s.n_total - s.nvar0);
        break;
    case 2: break;
    case 3: // :666-669
        st.fold_snp_num[1] = s.class_count[1];
        st.fold_snp_num[0] = s.n_total - s.nvar0 - st.fold_snp_num[1];
        st.NnzSnp = (long long)st.fold_snp_num[1];
        if (!p.fixpi) draw_pi();
        break;
    case 4: // :710-716
        st.fold_snp_num[1] = s.class_count[1];
        st.fold_snp_num[0] = s.n_total - s.nvar0 - st.fold_snp_num[1];
        st.NnzSnp = (long long)st.fold_snp_num[1];
        st.varg = (s.sum_g2 + p.s2varg * p.dfvara) / hs.chisq(p.dfvara + (double)st.NnzSnp);
        if (!p.fixpi) draw_pi();
        break;
    case 5: { // :738-741
        const double shape = p.shape0 + s.n_total - s.nvar0;
        const double rate = p.rate0 + s.sum_vargL / 2;
        st.lambda2 = hs.gamma(shape, 1 / rate);
        st.lambda = std::sqrt(st.lambda2);
        break;
    }
    case 6: { // :803-814 (class_count[0] already excludes the markers left out, :813)
        double nz = 0;
        for (int j = 0; j < p.n_fold; j++) st.fold_snp_num[j] = s.class_count[j];
        for (int j = 1; j < p.n_fold; j++) nz += st.fold_snp_num[j];
        st.NnzSnp = (long long)nz;
        st.varg = (s.sum_g2 + p.s2varg * p.dfvara) / hs.chisq(p.dfvara + (double)st.NnzSnp);
        for (int j = 0; j < p.n_fold; j++) st.vara_fold[j] = st.varg * p.fold[j];
        if (!p.fixpi) draw_pi();
        break;
    }
    }
}

// posterior inclusion probability from a count over nzct kept iterations: never exactly 1 (src/Bayes.cpp:1030, src/SBayesD.cpp:574)
static inline double hb_pip(double count, int nzct)
{
    double p = count / nzct;
    if (p == 1) p = (nzct - 1) / (double)nzct;
    return p;
}

// int n = mean(finite N) of the summary statistics (src/SBayesD.cpp:33-34, src/cg.cpp:13): column 3 of ss, leading dimension lds
static inline int hb_sumstat_n(const double *ss, long long lds, int m)
{
    double s = 0;
    int c = 0;
    for (int k = 0; k < m; k++)
        if (std::isfinite(ss[3 * lds + k])) { s += ss[3 * lds + k]; c++; }
    return (int)(s / std::max(1, c));
}

// ---- prior defaults, src/Bayes.cpp:327-374 and, the same expressions, src/SBayesD.cpp:117-170 ----
struct hb_prior_args { // the caller's has_* / value pairs, and what the run knows by now
    int has_vg, has_ve, has_dfve, has_s2vg, has_s2ve;
    double vg, ve, dfve, s2vg, s2ve;
    double dfvara, vary, h2;
    int nr;            // environmental random effects, which share the residual's half of var(y) (0 at the summary level)
    double Pi0, sumvx;
};
struct hb_priors {
    double vara, vare, dfvare, s2vara, varg, s2varg, s2vare, lambda2, lambda, shape0 = 1.1, rate0;
};
// vara_fold[0 .. n_fold) is filled too. The expressions are the reference's, operand for operand.
static inline hb_priors hb_prior_defaults(const hb_prior_args &p, const double *fold, int n_fold, double *vara_fold)
{
    hb_priors d;
    d.vara = p.has_vg ? p.vg : ((p.dfvara - 2) / p.dfvara) * p.vary * p.h2;
    d.vare = p.has_ve ? p.ve : p.vary * (1 - p.h2) / (p.nr + 1);
    d.dfvare = p.has_dfve ? p.dfve : -2;
    d.s2vara = p.has_s2vg ? p.s2vg : d.vara * (p.dfvara - 2) / p.dfvara;
    d.varg = d.vara / ((1 - p.Pi0) * p.sumvx);
    d.s2varg = d.s2vara / ((1 - p.Pi0) * p.sumvx);
    d.s2vare = p.has_s2ve ? p.s2ve : 0;
    const double R2 = (p.dfvara - 2) / p.dfvara;
    d.lambda2 = 2 * (1 - R2) / (R2)*p.sumvx;
    d.lambda = std::sqrt(d.lambda2);
    d.rate0 = (d.shape0 - 1) / d.lambda2;
    for (int j = 0; j < n_fold; j++) vara_fold[j] = (d.vara / ((1 - p.Pi0) * p.sumvx)) * fold[j];
    return d;
}

// ---- a sweep's parameters from the chain's state (hb_sweep_in) ----
// Pi, fold and vara_fold have n_fold entries, in the device's class order. thin < 1: never a thinned record (the summary level keeps its records on the host).
static inline hb_sweep_in hb_sweep_params(int model_index, int n_fold, const double *Pi, const double *fold, const double *vara_fold, double vare,
                                          double varg, double s2varg_df, double dfvara, double lambda, double lambda2, int iter, int nburn, int thin,
                                          bool always_in)
{
    hb_sweep_in in{};
    in.model_index = model_index;
    in.n_fold = n_fold;
    in.iter = iter;
    in.vare = vare;
    in.varg = varg;
    in.s2varg_df = s2varg_df;
    in.dfvara = dfvara;
    for (int j = 0; j < n_fold; j++) {
        in.logpi[j] = std::log(Pi[j]);
        in.fold[j] = fold[j];
        in.vara_fold[j] = vara_fold[j];
    }
    in.lambda = lambda;
    in.lambda2 = lambda2;
    in.count_pip = (iter >= nburn) && !always_in;
    in.store = thin >= 1 && (iter >= nburn) && ((iter + 1 - nburn) % thin == 0);
    return in;
}

// ---- the progress line of iteration iter (0-based), src/Bayes.cpp:884-914 and src/SBayesD.cpp:514-537 ----
// pi in the caller's class order (cls_of[]); extras: the model's own columns, preformatted with their trailing blanks (lambda for BayesL, va vb for
// BSLMM, veps for the epsilon block); vt: the denominator of h2; seconds: spent in the loop so far, from which the time left is extrapolated
static inline std::string hb_progress_line(int iter, int niter, long long NnzSnp, const double *Pi, const int *cls_of, int n_fold, const char *extras,
                                           double vara, double vare, double vt, double seconds)
{
    const int tt = (int)std::floor(seconds / (iter + 1) * (niter - iter));
    double pc[HB_MAX_FOLD] = {0};
    for (int j = 0; j < n_fold; j++) pc[cls_of[j]] = Pi[j];
    char buf[1024]; // (hb_line's own limit)
    int off = snprintf(buf, sizeof(buf), " %d %lld ", iter + 1, NnzSnp);
    for (int j = 0; j < n_fold; j++) off += snprintf(buf + off, sizeof(buf) - off, "%.4f ", pc[j]);
    snprintf(buf + off, sizeof(buf) - off, "%s%.4f %.4f %.4f %02dh%02dm%02ds", extras, vara, vare, vara / vt, tt / 3600, tt % 3600 / 60, tt % 3600 % 60);
    return buf;
}
