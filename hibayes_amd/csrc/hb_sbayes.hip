// hb_sbayes.hip — host side of hb_sbayes_run(): SBayesD() of the reference (src/SBayesD.cpp:5-609) as validation, prior defaults,
// the outer MCMC loop with its hyper-parameter draws and the posterior assembly; every m-long operation runs on the device
// (hb_sbayes.hpp). SURVEY §8 f4. hb_sbayes_run_sparse() is SBayesS() (src/SBayesS.cpp:21-640) through the same loop — the two
// functions of the reference share their validation, priors, hyper-parameter draws, records and assembly line for line — with
// the sweep of hb_sbayes_sparse.hip: what differs on the host is varediff (:131-141), vara and vary handed to the device every
// sweep, the sum of squared effects taken from the end-of-sweep reduction, and one console line (:222).
#include "hb_internal.hpp"
#include "hb_ldm.hpp"
#include "hb_model.hpp"
#include "hb_rng.hpp"
#include "hb_sbayes_sparse.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace {
struct sb_run {
    hb_ss_dev s;
    hb_sb_dev &d = s.b;
    double *h_ex = nullptr;
    hb_bufs mem;
    hipGraph_t graph = nullptr;
    hipGraphExec_t gexec = nullptr;
    double *h_acc = nullptr;
    hb_sweep_in *h_in = nullptr;
    ~sb_run()
    {
        if (gexec) (void)hipGraphExecDestroy(gexec);
        if (graph) (void)hipGraphDestroy(graph);
        mem.clear();
        if (d.stream) (void)hipStreamDestroy(d.stream);
    }
    template <typename T> int alloc(T **p, size_t count) { return mem.zeroed(p, count, d.stream); }
};
} // namespace

// hb_sbayes_run (H == nullptr: the matrix is args->ldm on the host), hb_sbayes_run_ldm (the matrix is the handle's dense device copy)
// and hb_sbayes_run_sparse (sparse: the handle's device CSC, SBayesS())
static int sbayes_run(const hb_sbayes_args *args, hb_ldm *H, hb_sbayes_out *o, bool sparse = false)
{
    if (!args || !o) return hb_fail(HB_ERR_INVALID, "hb_sbayes_run: null argument");
    const auto t_setup = hb_clk::now();
    const hb_sbayes_args &a = *args;
    const int m = a.m;
    if (H ? (m < 1 || !a.sumstat || a.ldm || a.ld_sumstat < m || H->m != m)
          : (m < 1 || !a.sumstat || !a.ldm || a.ld_sumstat < m || a.ld_ldm < m)) return hb_fail(HB_ERR_INVALID, "Number of SNPs not equals."); // :29-31
    if (!a.model) return hb_fail(HB_ERR_INVALID, "hb_sbayes_run: model is NULL");
    const std::string model = a.model;
    auto line = [&](const char *fmt, auto... xs) { hb_line(a.verbose, a.log, a.log_user, fmt, xs...); };
    // ---- validation and sizes, :28-74, same order and texts (hb_model.hpp) ----
    const int model_index = hb_model_index(model);
    const double *ss = a.sumstat;
    const int64_t lds = a.ld_sumstat;
    const int n = hb_sumstat_n(ss, lds, m); // :33-34
    std::string err;
    std::vector<double> Pi, fold_;
    std::vector<int> cls_of;
    bool fixpi = false, always_in = false;
    int rc = hb_mixture_take(model, a.Pi, a.n_pi, a.fold, a.n_fold, Pi, fold_, err);
    if (rc) return hb_fail(rc, err);
    const int n_fold = a.n_pi;
    const int niter = a.niter, nburn = a.nburn, thin = a.thin;
    if (thin < 1) return hb_fail(HB_ERR_INVALID, "hb_sbayes_run: thin must be >= 1");
    const int n_records = std::max(0, (niter - nburn) / thin);
    rc = hb_mixture_always_in(model, model_index, Pi, fixpi, always_in, err);
    if (!rc) rc = hb_mixture_order(model_index, Pi, fold_, cls_of, err);
    if (rc) return hb_fail(rc, err);
    long long NnzSnp = always_in ? m : 0;
    // ---- :95-115 ----
    std::vector<double> vx(m), xpx(m), xy(m, 0.0), yyi(m, 0.0), ifest(m, 1.0);
    for (int i = 0; i < m; i++) {
        vx[i] = H ? H->diag[i] : a.ldm[(size_t)i * a.ld_ldm + i];
        xpx[i] = vx[i] * n;
    }
    int count_y = 0;
    for (int k = 0; k < m; k++) {
        const double b = ss[1 * lds + k], se = ss[2 * lds + k], N = ss[3 * lds + k];
        if (std::isnan(b) || std::isnan(se) || std::isnan(N)) {
            ifest[k] = 0.0;
        } else {
            xy[k] = xpx[k] * b;
            yyi[k] = xpx[k] * (b * b + (N - 2) * se * se);
            count_y++;
        }
    }
    if (count_y == 0) return hb_fail(HB_ERR_INVALID, "Lack of SE.");
    const double yy = arma_sum(yyi.data(), m) / count_y;
    const double vary = yy / (n - 1);
    const double h2 = 0.5;
    // ---- priors, :117-170 (hb_model.hpp) ----
    const double dfvara_ = a.has_dfvg ? a.dfvg : 4;
    if (dfvara_ <= 2) return hb_fail(HB_ERR_INVALID, "dfvg should not be less than 2.");
    if (niter < nburn) return hb_fail(HB_ERR_INVALID, "Number of total iteration ('niter') shold be larger than burn-in ('nburn').");
    std::vector<double> vara_fold(n_fold), fold_snp_num(n_fold, 0.0), pi_sum(n_fold, 0.0);
    const hb_priors pr = hb_prior_defaults(hb_prior_args{a.has_vg, a.has_ve, a.has_dfve, a.has_s2vg, a.has_s2ve, a.vg, a.ve, a.dfve, a.s2vg, a.s2ve,
                                                         dfvara_, vary, h2, 0, Pi[0], arma_sum(vx.data(), m)}, fold_.data(), n_fold, vara_fold.data());
    double vara_ = pr.vara, vare_ = pr.vare, varg = pr.varg, lambda2 = pr.lambda2, lambda = pr.lambda;
    const double dfvare_ = pr.dfvare, s2vara_ = pr.s2vara, s2varg_ = pr.s2varg, s2vare_ = pr.s2vare, shape0 = pr.shape0, rate0 = pr.rate0;
    int nw = 0;
    if (a.windindx)
        for (int i = 0; i < m; i++) {
            if (a.windindx[i] < 1) return hb_fail(HB_ERR_INVALID, "hb_sbayes_run: window ids are 1-based");
            nw = std::max(nw, (int)a.windindx[i]);
        }

    // ---- device ----
    if (hb_device_count() <= 0) return hb_fail(HB_ERR_NO_DEVICE, "no HIP device available: the hibayes GPU engine has no CPU fallback");
    if (H && H->device != a.device) return hb_fail(HB_ERR_INVALID, "hb_sbayes_run_ldm: the LD matrix was built on another device");
    HB_HIP(hipSetDevice(a.device));
    sb_run R;
    hb_sb_dev &d = R.d;
    HB_HIP(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
    d.m = m;
    d.m_pad = (m + 255) / 256 * 256;
    d.n = n;
    d.seed = a.seed;
    d.nw = nw;
    if (sparse) { // adopted, not owned; nothing m x m exists on this route
        HB_TRY(hb_ldm_device_csc(H, &R.s.csc));
        HB_TRY(R.alloc(&R.s.varediff, d.m_pad));
        HB_TRY(R.alloc(&R.s.varei, d.m_pad));
        HB_TRY(R.alloc(&R.s.vxt, d.m_pad));
        HB_TRY(R.alloc(&R.s.sgn, d.m_pad));
        HB_TRY(R.alloc(&R.s.ex, 2));
        HB_TRY(R.alloc(&R.s.gtab, SS_GS));
        HB_TRY(R.alloc(&R.s.rd, 2));
        HB_TRY(R.alloc(&R.s.cursor, d.m_pad));
        HB_TRY(R.mem.pin(&R.h_ex, 2));
        HB_HIP(hipMemcpyAsync(R.s.vxt, vx.data(), sizeof(double) * m, hipMemcpyHostToDevice, d.stream));
        HB_TRY(hbk_ss_varediff(&R.s));
    } else if (H) { // adopted, not owned: the sweep only reads it
        const double *dl = nullptr;
        HB_TRY(hb_ldm_device_dense(H, &dl));
        d.ldm = const_cast<double *>(dl);
    } else {
        HB_TRY(R.alloc(&d.ldm, (size_t)m * m));
    }
    HB_TRY(R.alloc(&d.r_hat, d.m_pad));
    HB_TRY(R.alloc(&d.xy, d.m_pad));
    HB_TRY(R.alloc(&d.g, d.m_pad));
    HB_TRY(R.alloc(&d.xpx, d.m_pad));
    HB_TRY(R.alloc(&d.vx, d.m_pad));
    HB_TRY(R.alloc(&d.vargL, d.m_pad));
    HB_TRY(R.alloc(&d.thr, (size_t)d.m_pad * (HB_MAX_FOLD - 1)));
    HB_TRY(R.alloc(&d.invv, (size_t)d.m_pad * (HB_MAX_FOLD - 1)));
    HB_TRY(R.alloc(&d.sdz, (size_t)d.m_pad * (HB_MAX_FOLD - 1)));
    HB_TRY(R.alloc(&d.acc, HB_ACC_N));
    HB_TRY(R.alloc(&d.ev_gi, 512)); // SB_GS (hb_sbayes.hpp): the moves of one group
    HB_TRY(R.alloc(&d.ev_col, 512));
    HB_TRY(R.alloc(&d.ev_n, 1));
    HB_TRY(R.alloc(&d.tracker, d.m_pad));
    HB_TRY(R.alloc(&d.nzrate, d.m_pad));
    HB_TRY(R.alloc(&d.d_in, 1));
    if (nw) {
        HB_TRY(R.alloc(&d.wind, d.m_pad));
        HB_TRY(R.alloc(&d.wflag, nw));
        HB_TRY(R.alloc(&d.wppa, nw));
        HB_HIP(hipMemcpyAsync(d.wind, a.windindx, sizeof(uint32_t) * m, hipMemcpyHostToDevice, d.stream));
    }
    HB_TRY(R.mem.pin(&R.h_acc, HB_ACC_N));
    HB_TRY(R.mem.pin(&R.h_in, 1));
    if (!H) HB_HIP(hipMemcpy2DAsync(d.ldm, sizeof(double) * m, a.ldm, sizeof(double) * a.ld_ldm, sizeof(double) * m, m, hipMemcpyHostToDevice, d.stream));
    HB_HIP(hipMemcpyAsync(d.xy, xy.data(), sizeof(double) * m, hipMemcpyHostToDevice, d.stream));
    HB_HIP(hipMemcpyAsync(d.r_hat, xy.data(), sizeof(double) * m, hipMemcpyHostToDevice, d.stream)); // :108 r_hat = xy
    HB_HIP(hipMemcpyAsync(d.xpx, xpx.data(), sizeof(double) * m, hipMemcpyHostToDevice, d.stream));
    HB_HIP(hipMemcpyAsync(d.vx, ifest.data(), sizeof(double) * m, hipMemcpyHostToDevice, d.stream)); // (the kernels' "is this marker sampled" word)
    {
        std::vector<double> vl(m, varg); // :165-168 vargL.fill(varg)
        HB_HIP(hipMemcpyAsync(d.vargL, vl.data(), sizeof(double) * m, hipMemcpyHostToDevice, d.stream));
        HB_HIP(hipStreamSynchronize(d.stream));
    }
    o->n = n;
    o->count_y = count_y;
    o->nw = nw;
    o->n_records = n_records;
    const double setup_seconds = hb_since(t_setup);

    // ---- console, :190-246 ----
    line("Prior parameters:");
    line("    Model fitted at [%s]", model == "BayesRR" ? "Bayes Ridge Regression" : model.c_str());
    line(sparse ? "    Number of observations %d" : "    Population size %d", n);
    line("    Number of markers %d", m);
    line("    Number of markers used for analysis %d", count_y);
    line("    Total number of iteration %d", niter);
    line("    Total number of burn-in %d", nburn);
    line("    Phenotypic var %f", vary);
    line("    Genetic var %f", vara_);
    line("    Inv-Chisq gpar %f %f", dfvara_, s2vara_);
    line("    Residual var %f", vare_);
    line("    Inv-Chisq epar %f %f", dfvare_, s2vare_);
    line("    Marker var %f", varg);
    line("    Inv-Chisq alpar %f %f", dfvara_, s2varg_);
    if (nw) line("    Number of windows for GWAS analysis %d", nw);
    line("MCMC started: ");
    line(" Iter  NumNZSnp  pi  %sVg  Ve  h2  Timeleft", model == "BayesL" ? "Lambda  " : "");

    std::vector<double> s_alpha, g_sum(m, 0.0), g_host(m);
    if (a.store_alpha) s_alpha.assign((size_t)n_records * m, 0.0);
    double vara_sum = 0, vare_sum = 0, hsq_sum = 0, events_sum = 0;
    int count = 0, nzct = 0, iter = 0;
    const auto t_loop = hb_clk::now();
    for (iter = 0; iter < niter; iter++) {
        if (a.interrupt && a.interrupt(a.interrupt_user)) return hb_fail(HB_ERR_INTERRUPT, "interrupted");
        hb_stream hs(a.seed, hb_sub(HB_PURPOSE_HOST, (uint64_t)iter), 0);
        const hb_sweep_in in = hb_sweep_params(model_index, n_fold, Pi.data(), fold_.data(), vara_fold.data(), vare_, varg, s2varg_ * dfvara_, dfvara_,
                                               lambda, lambda2, iter, nburn, 0 /* never a device record */, always_in);
        *R.h_in = in;
        HB_HIP(hipMemcpyAsync(d.d_in, R.h_in, sizeof(hb_sweep_in), hipMemcpyHostToDevice, d.stream));
        if (sparse) { // varei = varediff[i] * vara_ + vare_ (:285) and the truncation's bound (:388)
            R.h_ex[0] = vara_;
            R.h_ex[1] = vary;
            HB_HIP(hipMemcpyAsync(R.s.ex, R.h_ex, sizeof(double) * 2, hipMemcpyHostToDevice, d.stream));
        }
        if (!R.gexec) { // one sweep = 2 ceil(m / 512) + 3 launches: captured once, replayed every iteration
            HB_HIP(hipStreamSynchronize(d.stream));
            HB_HIP(hipStreamBeginCapture(d.stream, hipStreamCaptureModeRelaxed));
            rc = sparse ? hbk_ss_enqueue_sweep(&R.s, model_index, n_fold) : hbk_sb_enqueue_sweep(&d, model_index, n_fold);
            hipError_t e = hipStreamEndCapture(d.stream, &R.graph);
            if (rc) return rc;
            if (e != hipSuccess) return hb_fail(HB_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
            HB_HIP(hipGraphInstantiate(&R.gexec, R.graph, nullptr, nullptr, 0));
        }
        HB_HIP(hipGraphLaunch(R.gexec, d.stream));
        if (in.count_pip && nw) HB_TRY(sparse ? hbk_ss_windows(&R.s) : hbk_sb_windows(&d));
        HB_HIP(hipMemcpyAsync(R.h_acc, d.acc, sizeof(double) * HB_ACC_N, hipMemcpyDeviceToHost, d.stream));
        HB_HIP(hipStreamSynchronize(d.stream));
        const double *acc = R.h_acc;
        events_sum += acc[HB_ACC_EVENTS];
        // :269-460; the sampled markers are the count_y with statistics (= m - nvar0: every marker is in one of the two counts)
        hb_draw_hyper(hs, hb_hyper_prior{model_index, n_fold, fixpi, dfvara_, s2varg_, shape0, rate0, fold_.data()},
                      hb_hyper_sums{acc[HB_ACC_SUMG2], acc[HB_ACC_SUMVARGL], acc + HB_ACC_COUNT0, (double)count_y, 0.0},
                      hb_hyper_state{varg, lambda, lambda2, NnzSnp, Pi.data(), vara_fold.data(), fold_snp_num.data()});
        vara_ = (acc[HB_ACC_SUMR] + s2vara_ * dfvara_) / hs.chisq(n + dfvara_);        // :468
        vare_ = (yy - acc[HB_ACC_SUMR2] + s2vare_ * dfvare_) / hs.chisq(n + dfvare_);  // :473
        if (vare_ < 0) vare_ = vara_ * 0.5;                                            // :474
        if (iter >= nburn) nzct++;
        if (iter >= nburn && (iter + 1 - nburn) % thin == 0 && count < n_records) { // :499-512
            if (!fixpi)
                for (int j = 0; j < n_fold; j++) {
                    if (o->s_pi) o->s_pi[(size_t)count * n_fold + cls_of[j]] = Pi[j];
                    pi_sum[j] += Pi[j];
                }
            if (o->s_Vg) o->s_Vg[count] = vara_;
            if (o->s_Ve) o->s_Ve[count] = vare_;
            if (o->s_h2) o->s_h2[count] = vara_ / (vara_ + vare_);
            vara_sum += vara_;
            vare_sum += vare_;
            hsq_sum += vara_ / (vara_ + vare_);
            HB_HIP(hipMemcpy(g_host.data(), d.g, sizeof(double) * m, hipMemcpyDeviceToHost));
            for (int i = 0; i < m; i++) g_sum[i] += g_host[i];
            if (a.store_alpha) std::memcpy(s_alpha.data() + (size_t)count * m, g_host.data(), sizeof(double) * m);
            count++;
        }
        if (a.verbose && a.outfreq > 0 && (iter + 1) % a.outfreq == 0) { // :514-537
            char lam[32] = {0};
            if (model == "BayesL") snprintf(lam, sizeof(lam), "%.4f ", lambda);
            line("%s", hb_progress_line(iter, niter, NnzSnp, Pi.data(), cls_of.data(), n_fold, lam, vara_, vare_, vara_ + vare_, hb_since(t_loop)).c_str());
        }
        if (count == n_records) {
            iter++;
            break;
        }
    }
    const double loop_seconds = hb_since(t_loop);
    // ---- posterior assembly, :541-580 ----
    const double Rn = (double)n_records;
    o->Vg = vara_sum / Rn;
    o->Ve = vare_sum / Rn;
    o->h2 = hsq_sum / Rn;
    if (o->alpha)
        for (int i = 0; i < m; i++) o->alpha[i] = g_sum[i] / Rn;
    if (a.store_alpha && o->s_alpha) std::memcpy(o->s_alpha, s_alpha.data(), sizeof(double) * s_alpha.size());
    if (!fixpi) {
        for (int j = 0; j < n_fold; j++) Pi[j] = pi_sum[j] / Rn;
    } else if (o->s_pi) {
        for (int r = 0; r < n_records; r++) {
            o->s_pi[(size_t)r * n_fold + 0] = Pi[0];
            o->s_pi[(size_t)r * n_fold + 1] = Pi[1];
        }
    }
    if (o->pi)
        for (int j = 0; j < n_fold; j++) o->pi[cls_of[j]] = Pi[j];
    if (o->pip) {
        if (always_in) for (int i = 0; i < m; i++) o->pip[i] = 1.0; // :571
        else {
            std::vector<uint32_t> nz(m);
            HB_HIP(hipMemcpy(nz.data(), d.nzrate, sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
            for (int i = 0; i < m; i++) o->pip[i] = hb_pip((double)nz[i], nzct); // :574
        }
    }
    if (nw && o->gwas) {
        std::vector<double> w(nw);
        HB_HIP(hipMemcpy(w.data(), d.wppa, sizeof(double) * nw, hipMemcpyDeviceToHost));
        for (int k = 0; k < nw; k++) o->gwas[k] = hb_pip(w[k], nzct);
    }
    if (o->r_hat) HB_HIP(hipMemcpy(o->r_hat, d.r_hat, sizeof(double) * m, hipMemcpyDeviceToHost));
    if (o->g_last) HB_HIP(hipMemcpy(o->g_last, d.g, sizeof(double) * m, hipMemcpyDeviceToHost));
    o->nzct = nzct;
    o->setup_seconds = setup_seconds;
    o->loop_seconds = loop_seconds;
    o->iters_done = iter;
    o->mean_events = iter > 0 ? events_sum / iter : 0;
    line("Posterior parameters:");
    line("    Genetic var %f", o->Vg);
    line("    Residual var %f", o->Ve);
    line("    Estimated h2 %f", o->h2);
    line("Finished: set-up %.2fs, MCMC %.2fs, %.1f sweeps/s", setup_seconds, loop_seconds, loop_seconds > 0 ? iter / loop_seconds : 0.0);
    return HB_OK;
}

extern "C" int hb_sbayes_run(const hb_sbayes_args *args, hb_sbayes_out *o) { return sbayes_run(args, nullptr, o); }

extern "C" int hb_sbayes_run_ldm(const hb_sbayes_args *args, hb_ldm *ldm, hb_sbayes_out *o)
{
    if (!ldm) return hb_fail(HB_ERR_INVALID, "hb_sbayes_run_ldm: null LD matrix handle");
    return sbayes_run(args, ldm, o);
}

extern "C" int hb_sbayes_run_sparse(const hb_sbayes_args *args, hb_ldm *ldm, hb_sbayes_out *o)
{
    if (!ldm) return hb_fail(HB_ERR_INVALID, "hb_sbayes_run_sparse: null LD matrix handle");
    return sbayes_run(args, ldm, o, true);
}
