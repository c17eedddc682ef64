// hb_run.hip — the host side of Bayes() (reference src/Bayes.cpp:60-1094) as a stepwise run object.
//
// What stays on the host, as in the reference: argument validation (:92-117, :293, :325, :357), prior
// defaults (:319-374), the outer MCMC loop (:477), the intercept / covariate / random-effect draws
// (:479-516), the hyper-parameter draws after the marker sweep (:603, :666-669, :710-716, :738-741,
// :803-814, :819-823), the thinned store (:848-882) and the posterior assembly (:919-1040).
// What runs on the device: everything that touches an n- or m-long vector (hb_kernels.hip).
// BSLMM's polygenic block (nk, :518-552) runs on the device too (hb_grm.hip) when Kival / Ki are given, and so does the single-step
// epsilon block (ne, :554-584; hb_epsl.hip) when epsl_y_J / epsl_Gi / epsl_index are.
//
// hb_bayes_run() == hb_run_create() + hb_run_step(niter) + hb_run_finish(); bench.py drives the
// three separately so that exactly K iterations sit between its barriers.
#include "hb_internal.hpp"
#include "hb_model.hpp"
#include "hb_rng.hpp"
#include "hb_runplan.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>

namespace {

// arma::var, N-1 (two-pass)
double var_n1(const double *v, size_t n)
{
    if (n < 2) return 0.0;
    const double mean = arma_sum(v, n) / n;
    double a2 = 0, a3 = 0;
    for (size_t i = 0; i < n; i++) {
        const double t = mean - v[i];
        a2 += t * t;
        a3 += t;
    }
    return (a2 - a3 * a3 / n) / (n - 1);
}

} // namespace

struct hb_run {
    // ---- arguments (deep copies: the caller's arrays need not outlive hb_run_create) ----
    hb_bayes_args a{};
    std::string model;
    std::vector<double> y, Cmat, Pi, fold_, g_init;
    bool has_warm = false;     // hb_bayes_args.warm: continue from a reported state instead of the prior defaults
    hb_warm_state warm_{};
    std::vector<double> warm_vargL;
    std::vector<uint32_t> wind;
    int n = 0, m = 0, model_index = 0, n_pi = 0, n_fold = 0, nc = 0, nr = 0, world = 1;
    bool fixpi = false, always_in = false, sharded = false;
    bool rowmode = false;      // hb_bayes_args.shard_rows: individuals sharded, exact digit-sum all-reduce per panel
    int64_t n_glob = 0, row_off = 0;
    int64_t m_global = 0;
    int niter = 0, nburn = 0, thin = 1, n_records = 0;
    // ---- device ----
    hb_ctx *c = nullptr;
    bool own_ctx = false;
    double *r0 = nullptr, *u0 = nullptr, *xbuf_own = nullptr, *xbuf = nullptr;
    hb_bufs mem; // r0, u0, xbuf_own
    size_t xcount = 0;
    // ---- state of the chain ----
    static constexpr double h2 = 0.5; // :119-124
    double vary = 0, sumvx = 0, ymean_glob = 0;
    std::vector<double> vx_host; // the markers' variances from marker_statistics to start_chain, where a g_init needs them (monomorphic markers start at zero)
    int nvar0 = 0, nw = 0, n_levels = 0;
    std::vector<double> beta, cpc, beta_sum, vr, vrtmp, vr_sum, zz, estR, estR_sum, vara_fold, fold_snp_num, pi_sum;
    std::vector<int32_t> zid, nlev, lev_first;
    std::vector<int> cls_of; // device class index -> the caller's (BayesR with an unsorted `fold`)
    double dfr = -1, s2r = 0, dfvara_ = 4, vara_ = 0, vare_ = 0, dfvare_ = -2, s2vara_ = 0, varg = 0, s2varg_ = 0,
           s2vare_ = 0, lambda2 = 0, lambda = 0, shape0 = 1.1, rate0 = 0, mu = 0;
    double sum_r = 0, sum_r2 = 0;
    int iter = 0, count = 0, nzct = 0;
    long long NnzSnp = 0;
    double mu_sum = 0, vara_sum = 0, vare_sum = 0, hsq_sum = 0, events_sum = 0, miss_sum = 0, redo_sum = 0;
    int sync_blocks = 1;       // runs of mat-vec groups per sweep, an exchange after each (hb_bayes_args.sync_blocks)
    bool recover_on = true;    // replay a sweep whose pipeline timed out (HB_RECOVER=0: fail the run, as before round 4)
    int wide_lv = 2;           // look-ahead groups of the point-mass models' wide geometry (HB_WIDE_LV=3: 3)
    bool no_adaptive_r = false, no_auto_bits = false; // HB_NO_ADAPTIVE_R, HB_NO_AUTO_BITS
    int pipeline_setup = -1;   // sharded runs: the context's pipeline switch as the ranks agreed on it in setup (checked at every step)
    hb_replay_state replay;    // sweeps replayed so far, and what the run has learnt about the device's waits (hb_runplan.hpp)
    hb_regime regime{};        // geometry by regime (plan_regime, hb_runplan.hpp): choose (Lv, D) per sweep from the previous sweep's moves
    int geo_cur = 0;           // 0: the wide geometry — (2 | 3, 7) for BayesB / C, (2, 2) for BayesR; 1: the narrow one — (2, 2), (2, 1)
    double last_events_pp = 0;
    bool done = false;
    double setup_seconds = 0, gram_seconds = 0, loop_seconds = 0;
    // MCMC sample stores kept inside the run (copied out by finish)
    std::vector<double> zb_, zl_, ch_; // this iteration's pre-drawn deviates for the covariate / random-effect blocks
    std::vector<double> s_mu, s_Vg, s_Ve, s_h2, s_pi, s_beta, s_Vr, s_r, s_alpha;
    // ---- BSLMM's polygenic block (:518-552): the state lives on the context (hb_ctx_poly_*), the records here ----
    bool poly = false, poly_finished = false;
    double va = 0, vb = 0;     // :715, :550
    std::vector<double> s_Va, s_Vb, k_mean, ghat;
    // ---- the single-step model's epsilon block (:554-584): the state lives on the context (hb_ctx_epsl_*), the records here ----
    bool epsl = false, epsl_finished = false, store_eps = true;
    int qe = 0, ne = 0;
    hb_epsl_gi epsl_gi{};
    std::vector<int64_t> eg_indptr;
    std::vector<int32_t> eg_indices;
    std::vector<double> eg_data, eps_yJ;
    std::vector<uint32_t> eps_index;
    double veps = 0, eps_J = 0;
    std::vector<double> s_Veps, s_J, s_eps, eps_mean;

    ~hb_run()
    {
        mem.clear(); // (buffers before the context's streams: hb_bufs.hpp)
        if (c && own_ctx) hb_ctx_destroy(c);
    }

    template <typename... A> void line(const char *fmt, A... xs) const { hb_line(a.verbose, a.log, a.log_user, fmt, xs...); }

    // sum over ranks of xbuf[0 .. xcount), on the sweep stream: RCCL inside the library when a communicator was given
    // (nothing but an enqueue), else the host language's callback (needs the stream quiesced on both sides)
    int exchange()
    {
        if (a.comm) return hb_comm_allreduce_f64(a.comm, xbuf, xcount, c->stream);
        HB_HIP(hipStreamSynchronize(c->stream));
        if (a.allreduce(xbuf, xcount, a.allreduce_user)) return hb_fail(HB_ERR_COMM, "all-reduce callback failed");
        return HB_OK;
    }

    int allreduce_host(double *vals, int cnt)
    { // a few host scalars through the device exchange buffer
        if (!sharded && !rowmode) return HB_OK;
        if (rowmode && world == 1 && !a.comm && !a.allreduce) return HB_OK; // (one shard: the sum over the ranks is the value itself)
        if ((size_t)cnt > xcount) return hb_fail(HB_ERR_INVALID, "allreduce_host: too many values");
        HB_HIP(hipMemsetAsync(xbuf, 0, sizeof(double) * xcount, c->stream));
        HB_HIP(hipMemcpyAsync(xbuf, vals, sizeof(double) * cnt, hipMemcpyHostToDevice, c->stream));
        int rc = exchange();
        if (rc) return rc;
        HB_HIP(hipMemcpyAsync(vals, xbuf, sizeof(double) * cnt, hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        return HB_OK;
    }

    // any number of host values summed over the ranks, in place (chunks of the exchange buffer)
    int allreduce_chunks(double *vals, size_t cnt)
    {
        for (size_t k0 = 0; k0 < cnt; k0 += xcount) {
            const int rc = allreduce_host(vals + k0, (int)std::min(xcount, cnt - k0));
            if (rc) return rc;
        }
        return HB_OK;
    }
    static int row_hook(void *user, double *vals, size_t cnt) { return static_cast<hb_run *>(user)->allreduce_chunks(vals, cnt); }
    // maximum over the ranks of one non-negative value each (a sum over one-hot slots)
    int allreduce_max(double *v)
    {
        std::vector<double> slot(world, 0.0);
        slot[a.rank] = *v;
        const int rc = allreduce_chunks(slot.data(), slot.size());
        for (double s : slot) *v = std::max(*v, s);
        return rc;
    }
    // K sums over ALL individuals, the same numbers on every rank AND for every number of shards: partial sums of fixed 256-row chunks
    // (add(i, p, nch) adds row i to its chunk's sums p[0], p[nch], ..., sequential inside a chunk), gathered over the ranks, added in chunk order
    template <int K, class F>
    int chunk_sums(double (&sum)[K], F add)
    {
        const size_t nch = (size_t)((n_glob + 255) / 256), c0 = (size_t)(row_off / 256);
        std::vector<double> part(K * nch, 0.0);
        for (int i = 0; i < n; i++) add(i, &part[c0 + (size_t)i / 256], nch);
        const int rc = allreduce_chunks(part.data(), part.size());
        if (rc) return rc;
        for (int k = 0; k < K; k++) {
            sum[k] = 0;
            for (size_t ch = 0; ch < nch; ch++) sum[k] += part[k * nch + ch];
        }
        return HB_OK;
    }
    // arma::var, two-pass, N - 1, from the second pass's sums over all individuals
    double var_glob(double a2, double a3) const { return n_glob > 1 ? (a2 - a3 * a3 / (double)n_glob) / (double)(n_glob - 1) : 0.0; }
    int row_stats_and_gram();
    int row_sums(double *sr, double *sr2, double *varu);
    int setup(const hb_bayes_args *args);
    // setup's parts, in the order it calls them
    int refuse_on_real(bool real) const;
    int take_args();
    int encode_random_effects();
    int take_model_args();
    int configure_device();
    int take_context();
    int open_exchange();
    int marker_statistics();
    int layout_and_regime();
    int prior_defaults();
    void console() const;
    int start_chain();
    int step();
    // step's parts, in the order it calls them
    int draw_before_sweep(hb_stream &hs);
    int choose_geometry();
    int sweep_with_replay(const hb_sweep_in &in, hb_sweep_out *so);
    int enqueue_sweep(const hb_sweep_in &in);
    int exchange_run(bool last);
    int take_sweep_results(hb_sweep_out *so);
    void draw_after_sweep(hb_stream &hs, const hb_sweep_out &so);
    int store_sample();
    void progress_line() const;
    int finish(hb_bayes_out *o);
};

// ---- row-sharded exact mode (hb_bayes_args.shard_rows) ----
// Marker statistics and Gram blocks are sums over individuals: the shards' integer sums are added up (exact in doubles), so
// xpx, vx and every Gram entry are the single-GPU numbers on every rank.
int hb_run::row_stats_and_gram()
{
    int rc = hb_ctx_marker_stats(c, nullptr, nullptr, nullptr, nullptr); // local S1 (c->s1), S2 (c->xpx), min / max
    if (rc) return rc;
    std::vector<double> s12((size_t)2 * m);
    HB_HIP(hipMemcpy(s12.data(), c->s1, sizeof(double) * m, hipMemcpyDeviceToHost));
    HB_HIP(hipMemcpy(s12.data() + m, c->xpx, sizeof(double) * m, hipMemcpyDeviceToHost));
    rc = allreduce_chunks(s12.data(), s12.size());
    if (rc) return rc;
    std::vector<double> vxh(m);
    const double N = (double)n_glob;
    for (int j = 0; j < m; j++) { // src/Bayes.cpp:310-317 from the exact integer sums: vx = (N S2 - S1^2) / (N (N - 1))
        const double num = N * s12[m + j] - s12[j] * s12[j];
        vxh[j] = (num == 0 || n_glob < 2) ? 0.0 : num / (N * (N - 1));
    }
    HB_HIP(hipMemcpy(c->xpx, s12.data() + m, sizeof(double) * m, hipMemcpyHostToDevice));
    HB_HIP(hipMemcpy(c->vx, vxh.data(), sizeof(double) * m, hipMemcpyHostToDevice));
    sumvx = arma_sum(vxh.data(), vxh.size());
    nvar0 = 0;
    for (double v : vxh) nvar0 += (v == 0.0);
    double lo = std::abs((double)c->xmin), hi = std::abs((double)c->xmax), neg = c->xmin < 0 ? 1.0 : 0.0;
    rc = allreduce_max(&lo);
    if (!rc) rc = allreduce_max(&hi);
    if (!rc) rc = allreduce_max(&neg);
    if (rc) return rc;
    c->xmax = (int)std::max(lo, hi); // (only max |x| matters from here on: the bound on max |yadj|, the Gram range check)
    c->xmin = neg != 0.0 ? -c->xmax : 0;
    rc = hb_ctx_build_gram(c, &gram_seconds);
    if (rc) return rc;
    const size_t cnt = (size_t)c->m_pad * c->P * (c->Lg + 1);
    std::vector<int32_t> gi(cnt);
    HB_HIP(hipMemcpy(gi.data(), c->gram, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost));
    std::vector<double> gd(cnt);
    for (size_t i = 0; i < cnt; i++) gd[i] = (double)gi[i];
    rc = allreduce_chunks(gd.data(), cnt);
    if (rc) return rc;
    for (size_t i = 0; i < cnt; i++) {
        if (std::fabs(gd[i]) >= 2147483647.0) return hb_fail(HB_ERR_UNSUPPORTED, "genotype codes too large for the exact int32 Gram matrix at this n");
        gi[i] = (int32_t)gd[i];
    }
    HB_HIP(hipMemcpy(c->gram, gi.data(), sizeof(int32_t) * cnt, hipMemcpyHostToDevice));
    return HB_OK;
}

// sum(yadj), yadj.yadj, var(u) over ALL individuals, the same numbers on every rank AND for every number of shards (chunk_sums)
int hb_run::row_sums(double *sr, double *sr2, double *varu)
{
    std::vector<double> r(n), u(n);
    int rc = hb_ctx_get_residual(c, r.data(), u.data());
    if (rc) return rc;
    double s[3], q[2];
    rc = chunk_sums(s, [&](int i, double *p, size_t nch) {
        p[0] += r[i];
        p[nch] = std::fma(r[i], r[i], p[nch]);
        p[2 * nch] += u[i];
    });
    if (rc) return rc;
    *sr = s[0];
    *sr2 = s[1];
    const double mean = s[2] / (double)n_glob;
    rc = chunk_sums(q, [&](int i, double *p, size_t nch) {
        const double d = mean - u[i];
        p[0] = std::fma(d, d, p[0]);
        p[nch] += d;
    });
    if (rc) return rc;
    *varu = var_glob(q[0], q[1]);
    return HB_OK;
}

int hb_run::setup(const hb_bayes_args *args)
{
    const auto t0 = hb_clk::now();
    a = *args;
    // the environment's switches, each read here and nowhere else
    if (const char *e = getenv("HB_RECOVER")) recover_on = atoi(e) != 0;
    if (const char *e = getenv("HB_WIDE_LV")) wide_lv = atoi(e) == 3 ? 3 : 2;
    no_adaptive_r = getenv("HB_NO_ADAPTIVE_R") != nullptr;
    no_auto_bits = getenv("HB_NO_AUTO_BITS") != nullptr;
    int rc = take_args();
    if (!rc) rc = encode_random_effects();
    if (!rc) rc = take_model_args();
    if (!rc) rc = configure_device();
    if (!rc) rc = prior_defaults();
    if (rc) return rc;
    console();
    rc = start_chain();
    if (rc) return rc;
    setup_seconds = hb_since(t0);
    return HB_OK;
}

// what the fp64 resident layout (real-valued genotypes, genotype_bits = 64) does not run with: asked as soon as the layout is known — from the
// arguments, and again once an upload under genotype_bits = 0 has chosen it
int hb_run::refuse_on_real(bool real) const
{
    if (!real) return HB_OK;
    if (rowmode) return hb_fail(HB_ERR_UNSUPPORTED, "shard_rows runs on the int8 layout, not on the fp64 resident layout (real-valued genotypes, genotype_bits = 64)");
    if (sharded || world > 1)
        return hb_fail(HB_ERR_UNSUPPORTED, "the fp64 resident layout (real-valued genotypes, genotype_bits = 64) is not sharded — it runs on one GPU only (comm / world > 1)");
    if (poly || model == "BSLMM")
        return hb_fail(HB_ERR_UNSUPPORTED, "BSLMM is not available on the fp64 resident layout (real-valued genotypes, genotype_bits = 64): the relationship matrix is an integer contraction");
    return HB_OK;
}

// the arguments' validation and deep copies, first half
int hb_run::take_args()
{
    n = a.n;
    m = a.m;
    if (n < 2 || m < 1 || !a.y) return hb_fail(HB_ERR_INVALID, "Number of individuals not equals.");
    if (!a.model) return hb_fail(HB_ERR_INVALID, "hb_bayes_run: model is NULL");
    model = a.model;
    a.model = model.c_str();
    y.assign(a.y, a.y + n);

    // ---- validation, same order and texts as src/Bayes.cpp:92-117 ----
    for (int i = 0; i < n; i++)
        if (std::isnan(y[i])) return hb_fail(HB_ERR_INVALID, "NAs are not allowed in y.");
    const bool have_x = a.X_f64 || a.X_i8;
    if (a.X_f64 && a.X_i8) return hb_fail(HB_ERR_INVALID, "hb_bayes_run: give X_f64 or X_i8, not both");
    if (!have_x && !a.ctx) return hb_fail(HB_ERR_INVALID, "hb_bayes_run: no genotype matrix (X_f64, X_i8 or a loaded ctx)");
    if (have_x && a.ctx) return hb_fail(HB_ERR_INVALID, "hb_bayes_run: a pre-loaded ctx excludes X_f64 / X_i8");
    if ((a.X_f64 && a.ld_f64 < n) || (a.X_i8 && a.ld_i8 < n)) return hb_fail(HB_ERR_INVALID, "Number of individuals not equals.");
    if (a.ctx && (a.ctx->n != n || a.ctx->m != m)) return hb_fail(HB_ERR_INVALID, "Number of individuals not equals.");
    model_index = model == "BSLMM" ? 4 : hb_model_index(model);
    std::string err;
    if (int rc = hb_mixture_take(model, a.Pi, a.n_pi, a.fold, a.n_fold, Pi, fold_, err)) return hb_fail(rc, err);
    n_pi = n_fold = a.n_pi;
    // BSLMM runs with both Kival and Ki, or on a context prepared by hb_ctx_poly_setup; anything else about them keeps the refusal (and its
    // text, which tests pin) from before the block existed
    poly = model == "BSLMM" && ((a.Ki && a.Kival) || (!a.Ki && !a.Kival && a.ctx && a.ctx->poly));
    if ((a.epsl_index || a.epsl_Gi || a.epsl_y_J) && model == "BSLMM")
        return hb_fail(HB_ERR_UNSUPPORTED, "the epsilon block is not available with BSLMM: the reference's ssbrm() has no such method");
    if (!poly && (a.Ki || a.Kival || model == "BSLMM")) return hb_fail(HB_ERR_UNSUPPORTED, "BSLMM (Ki/Kival) is not part of the GPU path");
    // the single-step epsilon block (:254-275): all three arguments or none, validated and copied here
    if (a.epsl_index || a.epsl_Gi || a.epsl_y_J) {
        if (!a.epsl_Gi) return hb_fail(HB_ERR_INVALID, "variance-covariance matrix should be provided for epsilon term.");
        if (!a.epsl_index || !a.epsl_y_J) return hb_fail(HB_ERR_INVALID, "hb_bayes_run: epsl_y_J, epsl_Gi and epsl_index go together");
        const hb_epsl_gi *G = static_cast<const hb_epsl_gi *>(a.epsl_Gi);
        if (int rc = hb_epsl_check(G, a.epsl_index, n)) return rc;
        for (int i = 0; i < n; i++)
            if (!std::isfinite(a.epsl_y_J[i])) return hb_fail(HB_ERR_INVALID, "epsl_y_J: a value is not finite");
        epsl = true;
        qe = G->q;
        ne = G->ne;
        eg_indptr.assign(G->indptr, G->indptr + qe + 1);
        eg_indices.assign(G->indices, G->indices + G->indptr[qe]);
        eg_data.assign(G->data, G->data + G->indptr[qe]);
        eps_yJ.assign(a.epsl_y_J, a.epsl_y_J + n);
        eps_index.assign(a.epsl_index, a.epsl_index + ne);
        epsl_gi = hb_epsl_gi{qe, ne, eg_indptr.data(), eg_indices.data(), eg_data.data()};
    }
    a.epsl_Gi = nullptr; // consumed
    a.epsl_index = nullptr;
    a.epsl_y_J = nullptr;

    world = a.world > 1 ? a.world : 1;
    if (a.comm) {
        world = hb_comm_world(a.comm);
        a.rank = hb_comm_rank(a.comm);
    }
    rowmode = a.shard_rows != 0;
    sharded = !rowmode && (world > 1 || a.comm != nullptr); // (a one-rank communicator still runs the exchange path)
    n_glob = rowmode ? a.n_global : n;
    row_off = rowmode ? a.row_offset : 0;
    if (rowmode) {
        if (!a.allreduce && !a.comm && world > 1) return hb_fail(HB_ERR_INVALID, "hb_bayes_run: shard_rows needs a communicator (comm or allreduce)");
        if (n_glob < n || row_off < 0 || row_off + n > n_glob || row_off % 256 || (row_off + n < n_glob && n % 256))
            return hb_fail(HB_ERR_INVALID, "hb_bayes_run: shard_rows needs row_offset and every shard but the last in multiples of 256 individuals");
        if (a.precise != 2) return hb_fail(HB_ERR_UNSUPPORTED, "shard_rows needs the exact fixed-point mat-vec (precise = 2): only integer sums are order-independent");
        if ((a.C && a.nc) || (a.R && a.nr)) return hb_fail(HB_ERR_UNSUPPORTED, "shard_rows: covariates and random effects are not part of the cross-check mode");
        if (a.genotype_bits == 2) return hb_fail(HB_ERR_UNSUPPORTED, "shard_rows runs on the int8 layout");
    }
    if (a.genotype_bits != 0 && a.genotype_bits != 8 && a.genotype_bits != 2 && a.genotype_bits != 64)
        return hb_fail(HB_ERR_INVALID, "hb_bayes_run: genotype_bits must be 0 (auto), 8, 2 or 64");
    if (int rc = refuse_on_real(a.genotype_bits == 64 || (a.ctx && a.ctx->layout == 64))) return rc;
    if (poly && (sharded || world > 1))
        return hb_fail(HB_ERR_UNSUPPORTED, "BSLMM: the polygenic block is not sharded — it runs on one GPU only (comm / world > 1)");
    if (poly && rowmode) return hb_fail(HB_ERR_UNSUPPORTED, "BSLMM: the polygenic block is not available with shard_rows");
    if (poly && a.warm) return hb_fail(HB_ERR_UNSUPPORTED, "BSLMM: a warm start (hb_warm_state) does not carry the polygenic state (k, vb)");
    if (epsl && (sharded || world > 1))
        return hb_fail(HB_ERR_UNSUPPORTED, "the epsilon block is not sharded — it runs on one GPU only (comm / world > 1)");
    if (epsl && rowmode) return hb_fail(HB_ERR_UNSUPPORTED, "the epsilon block is not available with shard_rows");
    if (epsl && a.warm) return hb_fail(HB_ERR_UNSUPPORTED, "the epsilon block: a warm start (hb_warm_state) does not carry its state (epsilon, J, veps)");
    sync_blocks = std::max(1, std::min(64, (int)a.sync_blocks));
    m_global = (!rowmode && (world > 1 || a.m_global > 0)) ? a.m_global : m;
    if (!rowmode && world > 1 && ((!a.allreduce && !a.comm) || m_global < m))
        return hb_fail(HB_ERR_INVALID, "hb_bayes_run: sharded run needs a communicator (comm or allreduce) and m_global");
    if (m_global < m) m_global = m;

    // ---- sizes, :119-124 ----
    vary = var_n1(y.data(), n); // (row-sharded mode: replaced by the variance over all shards once the exchange is up)
    niter = a.niter;
    nburn = a.nburn;
    thin = a.thin;
    if (thin < 1) return hb_fail(HB_ERR_INVALID, "hb_bayes_run: thin must be >= 1");
    n_records = std::max(0, (niter - nburn) / thin);

    // ---- covariates, :126-147 ----
    nc = a.C ? a.nc : 0;
    beta.assign(nc, 0.0);
    cpc.assign(nc, 0.0);
    beta_sum.assign(nc, 0.0);
    if (nc) {
        Cmat.assign(a.C, a.C + (size_t)n * nc);
        for (double v : Cmat)
            if (std::isnan(v)) return hb_fail(HB_ERR_INVALID, "Individuals with phenotypic value should not have missing covariates.");
        for (int i = 0; i < nc; i++) {
            const double *ci = Cmat.data() + (size_t)i * n;
            double s = 0;
            for (int k = 0; k < n; k++) s += ci[k] * ci[k];
            cpc[i] = s;
        }
    }
    return HB_OK;
}

int hb_run::encode_random_effects()
{
    // ---- environmental random effects, :149-201 with makeZ :29-57 ----
    nr = a.R ? a.nr : 0;
    dfr = a.has_dfvr ? a.dfvr : -1;
    s2r = a.has_s2vr ? a.s2vr : 0;
    vr.assign(nr, 0.0);
    vrtmp.assign(nr, vary * (1 - h2) / (nr + 1));
    vr_sum.assign(nr, 0.0);
    zid.assign((size_t)n * nr, 0);
    nlev.assign(nr, 0);
    lev_first.assign(nr, 0);
    for (int t = 0; t < nr; t++) {
        std::vector<std::string> vals(n);
        for (int k = 0; k < n; k++) {
            const char *s = a.R[(size_t)t * n + k];
            if (!s) return hb_fail(HB_ERR_INVALID, "Individuals with phenotypic value should not have missing environmental random effects.");
            vals[k] = s;
        }
        std::vector<std::string> lev(vals);
        std::stable_sort(lev.begin(), lev.end());
        lev.erase(std::unique(lev.begin(), lev.end()), lev.end());
        if ((int)lev.size() == n) return hb_fail(HB_ERR_INVALID, "number of class of environmental random effects should be less than population size.");
        if (lev.size() == 1) return hb_fail(HB_ERR_INVALID, "number of class of environmental random effects should be bigger than 1.");
        std::map<std::string, int> idx;
        for (size_t q = 0; q < lev.size(); q++) idx[lev[q]] = (int)q;
        lev_first[t] = n_levels;
        nlev[t] = (int)lev.size();
        zz.resize(n_levels + lev.size(), 0.0);
        for (int k = 0; k < n; k++) {
            const int q = idx[vals[k]];
            zid[(size_t)t * n + k] = q;
            zz[n_levels + q] += 1.0;
        }
        n_levels += (int)lev.size();
    }
    a.R = nullptr; // consumed
    estR.assign(n_levels, 0.0);
    estR_sum.assign(n_levels, 0.0);
    return HB_OK;
}

// validation and copies, second half: what depends on the model
int hb_run::take_model_args()
{
    // ---- :288-296 ----
    std::string err;
    if (int rc = hb_mixture_always_in(model, model_index, Pi, fixpi, always_in, err)) return hb_fail(rc, err);
    dfvara_ = a.has_dfvg ? a.dfvg : 4; // :319-326
    if (dfvara_ <= 2) return hb_fail(HB_ERR_INVALID, "dfvg should not be less than 2.");
    if (niter < nburn) return hb_fail(HB_ERR_INVALID, "Number of total iteration ('niter') shold be larger than burn-in ('nburn').");
    // BayesR runs as the chain of its classes sorted by fold; cls_of[] maps a class back to the caller's index (hb_model.hpp)
    if (int rc = hb_mixture_order(model_index, Pi, fold_, cls_of, err)) return hb_fail(rc, err);
    if (a.windindx) wind.assign(a.windindx, a.windindx + m);
    if (a.g_init) {
        g_init.assign(a.g_init, a.g_init + m);
        for (double v : g_init)
            if (!std::isfinite(v)) return hb_fail(HB_ERR_INVALID, "hb_bayes_run: g_init must be finite");
        a.g_init = nullptr; // consumed
    }
    if (a.warm) {
        has_warm = true;
        warm_ = *a.warm;
        // (advisor finding, round 5) hb_warm_state carries mu, vare, varg, pi, lambda2 and the per-marker variances — NOT the fixed-effect or
        // random-effect state (beta, the level effects, Vr): with C or R the run would restart those at their defaults beside warm marker
        // effects, which is not a continuation of the same chain. Refused rather than silently half-continued.
        if (a.nc > 0 || a.nr > 0)
            return hb_fail(HB_ERR_UNSUPPORTED, "hb_bayes_run: a warm start (hb_warm_state) does not carry the fixed / random effect state: not available with C or R");
        if (!(std::isfinite(warm_.mu) && warm_.vare > 0 && std::isfinite(warm_.vare)))
            return hb_fail(HB_ERR_INVALID, "hb_bayes_run: warm state needs a finite mu and vare > 0");
        if ((model_index == 1 || model_index == 4 || model_index == 6) && !(warm_.varg > 0 && std::isfinite(warm_.varg)))
            return hb_fail(HB_ERR_INVALID, "hb_bayes_run: warm state needs varg > 0 for this model");
        if (model_index == 5 && !(warm_.lambda2 > 0 && std::isfinite(warm_.lambda2)))
            return hb_fail(HB_ERR_INVALID, "hb_bayes_run: warm state needs lambda2 > 0 for BayesL");
        if (!always_in && !fixpi) {
            double sp = 0;
            for (int j = 0; j < n_fold; j++) {
                if (!(warm_.pi[j] > 0 && warm_.pi[j] < 1)) return hb_fail(HB_ERR_INVALID, "hb_bayes_run: warm state needs every pi in (0, 1)");
                sp += warm_.pi[j];
            }
            if (std::fabs(sp - 1.0) > 1e-9) return hb_fail(HB_ERR_INVALID, "hb_bayes_run: warm pi must sum to 1");
        }
        if (model_index == 5 && warm_.vargL) {
            warm_vargL.assign(warm_.vargL, warm_.vargL + m);
            for (double v : warm_vargL)
                if (!(v >= 0 && std::isfinite(v))) return hb_fail(HB_ERR_INVALID, "hb_bayes_run: warm vargL must be finite and >= 0");
        }
        warm_.vargL = nullptr;
        a.warm = nullptr; // consumed
    }
    return HB_OK;
}

// the caller's context, or one of the run's own with its geometry and the genotypes
int hb_run::take_context()
{
    int rc;
    if (a.ctx) {
        c = a.ctx;
        own_ctx = false;
        c->seed = a.seed;
        if (sharded) c->m_offset = a.m_offset; // (a single-process run keeps the context's own marker addressing)
        c->precise = a.precise;
        c->graph_model = -1;
    } else {
        hb_ctx_params cp{};
        cp.device = a.device;
        cp.n = n;
        cp.m = m;
        cp.panel = plan_panel(m, always_in, a.panel);
        cp.precise = a.precise;
        cp.m_offset = sharded ? a.m_offset : 0;
        cp.seed = a.seed;
        rc = hb_ctx_create(&cp, &c);
        if (rc) return rc;
        own_ctx = true;
        const hb_geometry ask = plan_default_geometry(model_index, n_fold, c->P, rowmode, wide_lv, no_adaptive_r);
        rc = hb_ctx_set_pipeline(c, ask.pipeline, ask.Lv, ask.D);
        if (rc) return rc;
        // integer genotypes take the int8 columns; real values — imputed dosages — the fp64 columns, where genotype_bits lets them (0: wherever the
        // matrix is not integer-valued within int8's range; 64: always, int8 input converted on the device; 8 / 2: never, the refusal stands)
        if (a.X_i8) {
            rc = hb_ctx_upload_genotype_i8(c, a.X_i8, a.ld_i8, 0, m);
            if (!rc && a.genotype_bits == 64) rc = hb_ctx_set_layout(c, 64, 0);
        } else if (a.genotype_bits == 64) rc = hb_ctx_upload_genotype_real(c, a.X_f64, a.ld_f64);
        else {
            rc = hb_ctx_upload_genotype_f64(c, a.X_f64, a.ld_f64, 0, m);
            if (rc == HB_ERR_UNSUPPORTED && a.genotype_bits == 0) {
                rc = refuse_on_real(true);
                if (!rc) rc = hb_ctx_upload_genotype_real(c, a.X_f64, a.ld_f64);
            }
        }
        if (rc) return rc;
    }
    a.X_i8 = nullptr;
    a.X_f64 = nullptr;
    return HB_OK;
}

// the context, its geometry, the exchange, the marker statistics, the resident layout, the Gram blocks and the regime: every decision is
// hb_runplan.hpp's, asked as soon as its facts are known and applied here
int hb_run::configure_device()
{
    int rc = take_context();
    if (rc) return rc;
    HB_HIP(hipSetDevice(c->device));
    if (poly && a.Ki) { // nk = n: K is read as n x n (:222)
        rc = hb_ctx_poly_setup(c, a.Kival, a.Ki, n, 0);
        if (rc) return rc;
    }
    a.Ki = a.Kival = nullptr; // consumed
    if (epsl) {
        const hb_epsl_desc d{&epsl_gi, eps_index.data(), eps_yJ.data()};
        rc = hb_ctx_epsl_setup(c, &d);
        if (rc) return rc;
        std::vector<int64_t>().swap(eg_indptr); // (the context holds its own copies)
        std::vector<int32_t>().swap(eg_indices);
        std::vector<double>().swap(eg_data);
    } else if (c->epsl) { // a caller's context that an earlier run left the block on: this run has none
        rc = hb_ctx_epsl_setup(c, nullptr);
        if (rc) return rc;
    }

    rc = open_exchange();
    if (!rc) rc = marker_statistics();
    if (!rc) rc = layout_and_regime();
    return rc;
}

// the resident layout, the Gram blocks, and whether and between which geometries the run follows the regime
int hb_run::layout_and_regime()
{
    int rc;
    auto layout = [&](size_t free_bytes) {
        return plan_layout(a.genotype_bits, own_ctx, rowmode, a.precise, model_index, n_fold, c->P, c->pipeline, c->xmin, c->xmax, no_auto_bits,
                           free_bytes, c->m_pad, c->ld, wide_lv);
    };
    int bits_run = c->layout == 64 ? 64 : layout(SIZE_MAX); // (fp64 columns stay what they are) a probe with all the memory there could be: the device is asked only where its answer decides
    if (bits_run == 2 && a.genotype_bits == 0) {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = 0;
        bits_run = layout(fr);
        if (bits_run != 2) (void)hipGetLastError(); // (a failed query must not stay behind as the thread's last error)
    }
    if (!c->gram_ready) {
        rc = hb_ctx_build_gram(c, &gram_seconds);
        if (rc) return rc;
    }
    if (bits_run == 2) { // the Gram blocks (built from the int8 columns) are in place: pack, drop the int8 copy
        rc = hb_ctx_set_layout(c, 2, 0);
        if (rc) return rc;
    }
    if (!own_ctx && c->adaptive && c->pipeline && c->home_d > 0 && (c->home_lv != c->Lv || c->home_d != c->D) && !rowmode) {
        // an adaptive context that an earlier run left in its narrow geometry: start from the geometry its owner set (round 6: a second fit
        // on the same context used to stay narrow for good, because only the wide geometry switches adaptivity on)
        rc = hb_ctx_switch_geometry(c, 1, c->home_lv, c->home_d);
        if (rc) return rc;
    }
    regime = plan_regime(model_index, n_fold, c->P, own_ctx, c->adaptive, hb_geometry{c->pipeline, c->Lv, c->D, c->L, c->NB}, c->Lg, no_adaptive_r);
    geo_cur = 0;
    if (regime.on) { // the first sweep: as many moves as markers are expected in the model (a cold start) or are in it
        double nz = 0;
        for (double gv : g_init) nz += gv != 0.0;
        if (g_init.empty()) nz = (1.0 - Pi[0]) * (double)m;
        last_events_pp = nz / std::max(1, c->npanels);
    }
    return HB_OK;
}

// the exchange buffers; row-sharded mode: its hook into the context, the per-panel kernels and var(y) over all shards
int hb_run::open_exchange()
{
    int rc;
    // (row-sharded mode: the shards hold different numbers of individuals, the message must not depend on n)
    xcount = rowmode ? hb_exchange_count(4096) : hb_exchange_count(n);
    if (sharded || rowmode) {
        if (a.exchange_buf) xbuf = static_cast<double *>(a.exchange_buf);
        else {
            HB_TRY(mem.get(&xbuf_own, xcount));
            xbuf = xbuf_own;
        }
        HB_TRY(mem.get(&r0, (size_t)n));
        HB_TRY(mem.get(&u0, (size_t)n));
    }
    if (rowmode) {
        c->row_reduce = &hb_run::row_hook;
        c->row_user = this;
        c->row_rank = a.rank;
        c->row_world = world;
        c->graph_model = -1;
        if (c->pipeline) { // (a pre-loaded context: the exchange needs the per-panel kernels)
            rc = hb_ctx_set_pipeline(c, 0, 0, 1);
            if (rc) return rc;
        }
        // var(y) over all shards, two-pass (arma::var), in the shard-count-independent order of chunk_sums()
        double tot[1], q[2];
        rc = chunk_sums(tot, [&](int i, double *p, size_t) { p[0] += y[i]; });
        if (rc) return rc;
        ymean_glob = tot[0] / (double)n_glob;
        rc = chunk_sums(q, [&](int i, double *p, size_t nch) {
            const double t = ymean_glob - y[i];
            p[0] += t * t;
            p[nch] += t;
        });
        if (rc) return rc;
        vary = var_glob(q[0], q[1]);
    }
    return HB_OK;
}

// marker statistics, :310-317, and what the ranks agree on about replaying a sweep
int hb_run::marker_statistics()
{
    int rc;
    vx_host.assign(g_init.empty() ? 0 : m, 0.0);
    if (rowmode) {
        rc = row_stats_and_gram();
        if (rc) return rc;
        if (!g_init.empty()) HB_HIP(hipMemcpy(vx_host.data(), c->vx, sizeof(double) * m, hipMemcpyDeviceToHost));
    } else
    rc = hb_ctx_marker_stats(c, nullptr, g_init.empty() ? nullptr : vx_host.data(), &sumvx, &nvar0);
    if (rc) return rc;
    if (sharded) { // marker shards: the statistics of all markers (row-sharded mode already holds the global ones)
        double sv[2] = {sumvx, (double)nvar0};
        rc = allreduce_host(sv, 2);
        if (rc) return rc;
        sumvx = sv[0];
        nvar0 = (int)sv[1];
    }
    if (sharded && world > 1) {
        // every rank must take the same replay decision (an aborting rank poisons the exchanged sums; a rank that would not replay
        // would fail while the others re-enter the all-reduce and hang): recovery is on only where ALL ranks have it — the
        // persistent pipeline available (the concurrency probe is per process) and HB_RECOVER not switched off
        double ok[1] = {(recover_on && c->pipeline) ? 1.0 : 0.0};
        rc = allreduce_host(ok, 1);
        if (rc) return rc;
        if (ok[0] < (double)world) {
            if (recover_on && c->pipeline)
                fprintf(stderr, "hibayes_gpu: rank %d: sweep replay switched off — not every rank can replay (HB_RECOVER / pipeline availability differ)\n", a.rank);
            recover_on = false;
        }
        pipeline_setup = c->pipeline ? 1 : 0;
    }
    return HB_OK;
}

int hb_run::prior_defaults()
{
    int rc;
    // ---- prior defaults, :327-374 (hb_model.hpp) ----
    vara_fold.assign(n_fold, 0.0);
    fold_snp_num.assign(n_fold, 0.0);
    pi_sum.assign(n_fold, 0.0);
    const hb_priors pr = hb_prior_defaults(hb_prior_args{a.has_vg, a.has_ve, a.has_dfve, a.has_s2vg, a.has_s2ve, a.vg, a.ve, a.dfve, a.s2vg, a.s2ve,
                                                         dfvara_, vary, h2, nr, Pi[0], sumvx}, fold_.data(), n_fold, vara_fold.data());
    vara_ = pr.vara, vare_ = pr.vare, dfvare_ = pr.dfvare, s2vara_ = pr.s2vara, varg = pr.varg, s2varg_ = pr.s2varg, s2vare_ = pr.s2vare;
    lambda2 = pr.lambda2, lambda = pr.lambda, shape0 = pr.shape0, rate0 = pr.rate0;
    {
        std::vector<double> g0(m, 0.0), vl(m, varg);
        std::vector<uint8_t> t0v(m, 0);
        rc = hb_ctx_set_effects(c, g0.data(), t0v.data(), warm_vargL.empty() ? vl.data() : warm_vargL.data()); // vargL.fill(varg), :364-368
        if (rc) return rc;
        HB_HIP(hipMemsetAsync(c->nzrate, 0, sizeof(uint32_t) * (size_t)c->m_pad, c->stream));
        HB_HIP(hipMemsetAsync(c->alpha_sum, 0, sizeof(double) * (size_t)c->m_pad, c->stream));
        HB_HIP(hipMemsetAsync(c->alpha_sq, 0, sizeof(double) * (size_t)c->m_pad, c->stream));
    }
    if (!wind.empty()) {
        for (int i = 0; i < m; i++) nw = std::max(nw, (int)wind[i]);
        if (world > 1) { // window ids are global: every rank needs the same nw (max over ranks)
            if ((size_t)world > xcount) return hb_fail(HB_ERR_INVALID, "too many ranks for the exchange buffer");
            double nwmax = nw;
            rc = allreduce_max(&nwmax);
            if (rc) return rc;
            nw = (int)nwmax;
        }
        rc = hb_ctx_set_windows(c, wind.data(), nw);
        if (rc) return rc;
    } else {
        rc = hb_ctx_set_windows(c, nullptr, 0);
        if (rc) return rc;
    }
    rc = hb_ctx_set_covariates(c, nc ? Cmat.data() : nullptr, nc);
    if (rc) return rc;
    rc = hb_ctx_set_levels(c, nr ? zid.data() : nullptr, nr, nr ? nlev.data() : nullptr);
    if (rc) return rc;
    rc = hb_ctx_blocks_setup(c, cpc.data(), zz.data(), vrtmp.data());
    if (rc) return rc;
    return HB_OK;
}

void hb_run::console() const
{
    // ---- console, :393-461 ----
    line("Prior parameters:");
    line("    Model fitted at [%s]", model == "BayesRR" ? "Bayes Ridge Regression" : model.c_str());
    line("    Number of observations %d", n);
    line("    Number of covariates %d", nc + 1);
    line("    Number of envir-random effects %d", nr);
    line("    Number of markers %lld", (long long)m_global);
    line("    Total number of iteration %d", niter);
    line("    Total number of burn-in %d", nburn);
    line("    Frequency of collecting %d", thin);
    line("    Phenotypic var %f", vary);
    line("    Genetic var %f", vara_);
    line("    Inv-Chisq gpar %f %f", dfvara_, s2vara_);
    line("    Residual var %f", vare_);
    line("    Inv-Chisq epar %f %f", dfvare_, s2vare_);
    line("    Marker var %f", varg);
    line("    Inv-Chisq alpar %f %f", dfvara_, s2varg_);
    if (nw) line("    Number of windows for GWAS analysis %d", nw);
    if (world > 1 && always_in)
        line("    WARNING: %d marker shards with a model in which every marker moves every sweep (%s): shards are stale with "
             "respect to each other inside a sweep, variance components are biased (DESIGN.md section 8)", world, model.c_str());
    line("MCMC started: ");
    line(" Iter  NumNZSnp  pi  %sVg  Ve  h2  Timeleft", model == "BayesL" ? "Lambda  " : "");
}

// the chain's first state: a continued chain's scalars, the intercept, the residual and its sums, the sample stores
int hb_run::start_chain()
{
    int rc;
    // ---- warm state: the scalars of a chain that is continued (the constants above stay the cold run's) ----
    if (has_warm) {
        vare_ = warm_.vare;
        if (model_index == 1 || model_index == 4 || model_index == 6) varg = warm_.varg;
        if (model_index == 6)
            for (int j = 0; j < n_fold; j++) vara_fold[j] = varg * fold_[j]; // :808
        if (model_index == 5) {
            lambda2 = warm_.lambda2;
            lambda = std::sqrt(lambda2);
        }
        if (!always_in && !fixpi)
            for (int j = 0; j < n_fold; j++) Pi[j] = warm_.pi[cls_of[j]]; // (internal class j is the caller's cls_of[j])
    }

    // ---- :469-472 ----
    mu = has_warm ? warm_.mu : (rowmode ? ymean_glob : arma_sum(y.data(), n) / n);
    {
        std::vector<double> yadj(n), zero(n, 0.0);
        for (int i = 0; i < n; i++) yadj[i] = y[i] - mu;
        if (!g_init.empty()) {
            // warm start: monomorphic markers are never visited by the sweep (:589), so they start (and stay) at zero
            std::vector<uint8_t> trk(m, 0);
            for (int i = 0; i < m; i++) {
                if (vx_host[i] == 0.0) g_init[i] = 0.0;
                trk[i] = g_init[i] != 0.0;
            }
            std::vector<double>().swap(vx_host); // (needed no longer: not kept for the length of the run)
            rc = hb_ctx_set_effects(c, g_init.data(), trk.data(), nullptr);
            if (rc) return rc;
            rc = hb_ctx_matvec(c, g_init.data(), zero.data()); // u = X g
            if (rc) return rc;
            if (sharded) { // every rank starts from the residual of ALL shards' effects (u and yadj are replicated)
                rc = allreduce_host(zero.data(), n);
                if (rc) return rc;
            }
            for (int i = 0; i < n; i++) yadj[i] -= zero[i];
        }
        rc = hb_ctx_set_residual(c, yadj.data(), zero.data());
        if (rc) return rc;
    }
    if (rowmode) {
        double vu = 0;
        rc = row_sums(&sum_r, &sum_r2, &vu);
    } else {
        rc = hb_ctx_residual_sums(c, &sum_r, &sum_r2);
    }
    if (rc) return rc;
    NnzSnp = always_in ? m_global : 0;
    s_mu.assign(n_records, 0.0);
    s_Vg.assign(n_records, 0.0);
    s_Ve.assign(n_records, 0.0);
    s_h2.assign(n_records, 0.0);
    s_pi.assign((size_t)n_records * n_fold, 0.0);
    s_beta.assign((size_t)n_records * nc, 0.0);
    s_Vr.assign((size_t)n_records * nr, 0.0);
    s_r.assign((size_t)n_records * n_levels, 0.0);
    if (a.store_alpha) s_alpha.assign((size_t)n_records * m, 0.0);
    if (poly) {
        rc = hb_poly_reset(c); // k = 0 (:228-230)
        if (rc) return rc;
        s_Va.assign(n_records, 0.0);
        s_Vb.assign(n_records, 0.0);
    }
    if (epsl) {
        rc = hb_epsl_reset(c); // epsilon = 0, J = 0 (:251, :268)
        if (rc) return rc;
        s_Veps.assign(n_records, 0.0);
        s_J.assign(n_records, 0.0);
        if (store_eps) s_eps.assign((size_t)n_records * qe, 0.0);
    }
    return HB_OK;
}

// one iteration of the loop at src/Bayes.cpp:477-917, in the reference's order; the parts follow
int hb_run::step()
{
    if (done || iter >= niter) {
        done = true;
        return HB_OK;
    }
    const auto t0 = hb_clk::now();
    HB_HIP(hipSetDevice(c->device));
    if (a.interrupt && a.interrupt(a.interrupt_user)) return hb_fail(HB_ERR_INTERRUPT, "interrupted");
    hb_stream hs(a.seed, hb_sub(HB_PURPOSE_HOST, (uint64_t)iter), 0);
    HB_TRY(draw_before_sweep(hs)); // :479-584
    // ---------------- marker sweep on the device, :586-816 ----------------
    const hb_sweep_in in = hb_sweep_params(model_index, n_fold, Pi.data(), fold_.data(), vara_fold.data(), vare_, varg, s2varg_ * dfvara_, dfvara_, lambda,
                                           lambda2, iter, nburn, thin, always_in);
    hb_sweep_out so{};
    HB_TRY(choose_geometry());
    HB_TRY(sweep_with_replay(in, &so));
    HB_TRY(take_sweep_results(&so));
    draw_after_sweep(hs, so); // :603-823
    if (iter >= nburn) nzct++; // :826-845 (the per-marker counters themselves live on the device)
    if (in.store && count < n_records) HB_TRY(store_sample()); // :848-882
    loop_seconds += hb_since(t0);
    if (a.verbose && a.outfreq > 0 && (iter + 1) % a.outfreq == 0) progress_line(); // :884-914
    iter++;
    if (count == n_records || iter >= niter) done = true; // :916
    return HB_OK;
}

// the draws and enqueues before the sweep, in the reference's order on the host stream hs (that order is part of the chain)
int hb_run::draw_before_sweep(hb_stream &hs)
{
    // sample intercept, :479-482
    const double ng = (double)n_glob; // (= n unless the individuals are sharded)
    const double mu_ = -(sum_r / ng + std::sqrt(vare_ / ng) * hs.norm());
    mu -= mu_;
    HB_TRY(hb_ctx_residual_shift(c, mu_));

    // covariates (:484-494) and environmental random effects (:496-516): enqueued as device kernels. Their deviates do not
    // depend on the data, so they are drawn here first, in the reference's order — one normal per covariate, then per term
    // its level normals followed by its chisq — and the state comes back with the sweep's fetch: one host sync per iteration
    if (nc + nr) {
        zb_.resize(nc);
        zl_.resize(n_levels);
        ch_.resize(nr);
        for (int i = 0; i < nc; i++) zb_[i] = hs.norm();
        for (int t = 0; t < nr; t++) {
            for (int q = 0; q < nlev[t]; q++) zl_[lev_first[t] + q] = hs.norm();
            ch_[t] = hs.chisq(nlev[t] + dfr);
        }
        HB_TRY(hb_ctx_blocks_step(c, vare_, zb_.data(), zl_.data(), ch_.data(), dfr, s2r));
    }
    // BSLMM's polygenic block (:518-552), enqueued like the blocks above: its normals are drawn on the device, its chisq (:547) here, at the
    // reference's place in the host stream; vb and the check of :533 come back with the sweep's fetch. Before the sweep's snapshot
    // (sweep_with_replay): a replayed sweep restarts from the residual this block left.
    if (poly) {
        const double chis = hs.chisq(dfvara_ + (double)n);
        HB_TRY(hb_ctx_poly_step(c, vare_, iter == 0 ? vara_ : -1.0, a.seed, iter, chis, s2vara_ * dfvara_)); // (vbtmp = vara_, :333)
    }
    // the single-step epsilon block (:554-584), enqueued the same way and at the same place: the J draw's normal (:559) and the chisq of :579
    // from the host stream here, the rows' normals on the device; veps and J come back with the sweep's fetch
    if (epsl) {
        const double zJ = hs.norm();
        const double chis = hs.chisq(dfvara_ + (double)qe);
        HB_TRY(hb_ctx_epsl_step(c, vare_, iter == 0 ? vara_ : -1.0, a.seed, iter, zJ, chis, s2vara_ * dfvara_)); // (vepstmp = vara_, :332)
    }
    return HB_OK;
}

// geometry by regime (hb_runplan.hpp), when the context is ours or its owner asked for it
int hb_run::choose_geometry()
{
    if (!regime.on) return HB_OK;
    const int want = regime_next(regime, geo_cur, last_events_pp); // (moves per panel of the previous sweep on this shard)
    if (want != geo_cur) {
        HB_TRY(hb_ctx_switch_geometry(c, 1, regime.Lv[want], regime.D[want]));
        geo_cur = want;
    }
    return HB_OK;
}

namespace {
// Whatever way a sweep ends, the context gets back the wait bound and the geometry it came with (a caller-owned context
// outlives the run): a scope guard, not a line after the loop that the error returns inside it would skip.
struct restore_ctx {
    hb_ctx *c;
    int timeout_ms;
    int geo[4] = {0, 0, 0, 0};
    bool fell_back = false;
    ~restore_ctx()
    {
        c->timeout_ms = timeout_ms;
        if (fell_back) (void)hb_ctx_force_geometry(c, geo[0], geo[1], geo[2]);
    }
};
} // namespace

// The sweep, and its replay when it aborts.
// A sweep whose pipeline gave up waiting (HB_ERR_ABORTED: every wait is bounded) is replayed from the state
// saved here: effects, residual, u and the posterior counters, a few MB copied by one kernel. The draws are counter-based, so the
// replay is the same chain. A second failure of the same sweep replays it on the event-ordered per-panel kernels, which wait
// for nothing on the device; sharded, the abort reaches every rank through the exchange and all of them replay. The policy — the wait bounds,
// when to fall back, when to give up, when a device counts as slow — is hb_runplan.hpp's ("replaying an aborted sweep"); it is asked and applied here.
int hb_run::sweep_with_replay(const hb_sweep_in &in, hb_sweep_out *so)
{
    // (advisor finding, round 5) the replay decision was agreed by all ranks in setup on the context's pipeline switch as it was then; a caller that flips
    // it on one rank afterwards (hb_ctx_set_pipeline between steps) would make that rank's decision differ and the others hang in the exchange: refuse loudly.
    // (The adaptive geometry changes Lv and D, never this switch; the replay's own fallback flips it inside this function and puts it back.)
    if (pipeline_setup >= 0 && (c->pipeline ? 1 : 0) != pipeline_setup)
        return hb_fail(HB_ERR_INVALID, "the context's pipeline switch changed during a sharded run (the ranks agreed on their replay decision with the setting at set-up)");
    const bool recover = replay_enabled(recover_on, c->pipeline, rowmode);
    restore_ctx guard{c, c->timeout_ms};
    c->timeout_ms = replay_first_wait_ms(recover, c->timeout_env, c->timeout_ms, replay);
    if (recover) HB_TRY(hb_ctx_snapshot(c, model_index, in.store != 0, in.count_pip != 0));
    for (int attempt = 0;; attempt++) {
        HB_TRY(enqueue_sweep(in));
        const int rc = hb_ctx_sweep_end(c, so);
        if (rc != HB_ERR_ABORTED) return rc;
        const hb_replay_step next = replay_after_abort(recover, attempt, guard.fell_back, iter, c->timeout_ms, replay);
        if (!next.replay) return rc;
        replay = next.state;
        // the switch to the per-panel kernels is forced past HB_PIPELINE / HB_LOOKAHEAD / HB_DOTGROUP: a tuning variable must not turn the
        // fall-back into a third try of the pipeline that just stalled twice
        bool per_panel = guard.fell_back;
        if (next.to_per_panel) {
            (void)hb_ctx_get_pipeline(c, &guard.geo[0], &guard.geo[1], &guard.geo[2], &guard.geo[3]);
            HB_TRY(hb_ctx_force_geometry(c, 0, 0, 1));
            guard.fell_back = true;
            per_panel = c->pipeline == 0;
        }
        fprintf(stderr, "hibayes_gpu: iteration %d: %s — state restored, replaying the sweep%s\n", iter + 1, hb_last_error(),
                per_panel ? " on the per-panel kernels" : "");
        HB_TRY(hb_ctx_restore(c));
        c->timeout_ms = next.timeout_ms;
    }
}

// One attempt at the sweep, in sync_blocks runs of mat-vec groups (1: the whole sweep). After each run the shards sum their residual
// deltas (n doubles; u moves by the negative) — and, after the last one, the 16 scalar sums — all enqueued on the sweep
// stream behind the run itself; the iteration's only host synchronisation is the fetch that follows (hb_ctx_sweep_end).
int hb_run::enqueue_sweep(const hb_sweep_in &in)
{
    for (int b = 0; b < sync_blocks; b++) {
        if (sharded) {
            HB_HIP(hipMemcpyAsync(r0, c->r, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
            HB_HIP(hipMemcpyAsync(u0, c->u, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
        }
        HB_TRY(hb_ctx_sweep_range(c, &in, b, sync_blocks));
        if (sharded) HB_TRY(exchange_run(b == sync_blocks - 1));
    }
    return HB_OK;
}

// the sharded exchange of one run: pack, poison, exchange, unpack, and the sums after the last
int hb_run::exchange_run(bool last)
{
    HB_TRY(hbk_delta_pack(c, r0, u0, xbuf));
    // (the sums ride along every time — the message has one shape — but only the last run's are the sweep's)
    HB_HIP(hipMemcpyAsync(xbuf + (size_t)n, c->acc, sizeof(double) * HB_ACC_N, hipMemcpyDeviceToDevice, c->stream));
    HB_TRY(hbk_abort_poison(c, xbuf + (size_t)n));
    HB_TRY(exchange());
    HB_TRY(hbk_delta_unpack(c, r0, u0, xbuf));
    if (last) {
        HB_HIP(hipMemcpyAsync(c->acc, xbuf + (size_t)n, sizeof(double) * HB_ACC_N, hipMemcpyDeviceToDevice, c->stream));
        HB_TRY(hbk_reduce_ru(c));
    }
    return HB_OK;
}

// the sweep's results into the chain's state
int hb_run::take_sweep_results(hb_sweep_out *so)
{
    events_sum += so->n_events;
    last_events_pp = so->n_events / ((double)std::max(1, world) * std::max(1, c->npanels));
    miss_sum += so->n_cache_miss;
    redo_sum += so->n_redo;
    sum_r = so->sum_r;
    sum_r2 = so->sum_r2;
    if (rowmode) { // the three n-long reductions over all shards (the sweep's own ones saw this shard's rows only)
        if (c->row_failed) return hb_fail(HB_ERR_COMM, "row-sharded mode: an all-reduce inside the sweep failed");
        HB_TRY(row_sums(&sum_r, &sum_r2, &so->var_u));
    }
    if (nc + nr) { // the block state arrived with the sweep's fetch
        const double *h = c->h_blk;
        std::copy(h, h + nc, beta.begin());
        std::copy(h + nc, h + nc + n_levels, estR.begin());
        std::copy(h + nc + n_levels, h + nc + n_levels + nr, vrtmp.begin());
        std::copy(h + nc + n_levels + nr, h + nc + n_levels + 2 * nr, vr.begin());
    }
    if (poly) {
        const double *ps = hb_poly_host_state(c);
        if (ps[2] != 0.0)
            return hb_fail(HB_ERR_INVALID, "matrix is not positive definite, try to specify parameter 'lambda' with a small value, eg: 0.001 or bigger"); // :533
        vb = ps[0];
    }
    if (epsl) {
        const double *es = hb_epsl_host_state(c);
        veps = es[0];
        eps_J = es[2];
    }
    return HB_OK;
}

// hyper-parameters after the sweep (hb_model.hpp), then the two variances
void hb_run::draw_after_sweep(hb_stream &hs, const hb_sweep_out &so)
{
    hb_draw_hyper(hs, hb_hyper_prior{model_index, n_fold, fixpi, dfvara_, s2varg_, shape0, rate0, fold_.data()},
                  hb_hyper_sums{so.sum_g2, so.sum_vargL, so.class_count, (double)m_global, (double)nvar0},
                  hb_hyper_state{varg, lambda, lambda2, NnzSnp, Pi.data(), vara_fold.data(), fold_snp_num.data()});
    if (poly) va = varg; // :715
    vara_ = so.var_u;                                                                 // :819
    vare_ = (sum_r2 + s2vare_ * dfvare_) / hs.chisq((double)n_glob + dfvare_);  // :823
}

// thinned store, :848-882
int hb_run::store_sample()
{
    s_mu[count] = mu;
    mu_sum += mu;
    if (!fixpi)
        for (int j = 0; j < n_fold; j++) {
            s_pi[(size_t)count * n_fold + j] = Pi[j];
            pi_sum[j] += Pi[j];
        }
    s_Vg[count] = vara_;
    s_Ve[count] = vare_;
    if (poly) { // :854-858
        s_Va[count] = va;
        s_Vb[count] = vb;
        HB_TRY(hbk_poly_accumulate(c));
    }
    if (epsl) { // :873-877
        s_Veps[count] = veps;
        s_J[count] = eps_J;
        HB_TRY(hbk_epsl_accumulate(c, store_eps ? s_eps.data() + (size_t)count * qe : nullptr));
    }
    vara_sum += vara_;
    vare_sum += vare_;
    if (a.store_alpha) HB_TRY(hb_ctx_get_effects(c, s_alpha.data() + (size_t)count * m, nullptr, nullptr));
    for (int i = 0; i < nc; i++) {
        s_beta[(size_t)count * nc + i] = beta[i];
        beta_sum[i] += beta[i];
    }
    double vt = vara_ + vare_;
    for (int t = 0; t < nr; t++) {
        vt += vr[t];
        s_Vr[(size_t)count * nr + t] = vr[t];
        vr_sum[t] += vr[t];
    }
    for (int q = 0; q < n_levels; q++) {
        s_r[(size_t)count * n_levels + q] = estR[q];
        estR_sum[q] += estR[q];
    }
    s_h2[count] = vara_ / vt;
    hsq_sum += vara_ / vt;
    count++;
    return HB_OK;
}

// the console line, :884-914 (hb_model.hpp formats it)
void hb_run::progress_line() const
{
    double vt = vara_ + vare_;
    for (int t = 0; t < nr; t++) vt += vr[t];
    char lam[32] = {0};
    if (model == "BayesL") snprintf(lam, sizeof(lam), "%.4f ", lambda);
    if (poly) snprintf(lam, sizeof(lam), "%.4f %.4f ", va, vb); // :901
    if (epsl) snprintf(lam + strlen(lam), sizeof(lam) - strlen(lam), "%.4f ", veps); // :908
    line("%s", hb_progress_line(iter, niter, NnzSnp, Pi.data(), cls_of.data(), n_fold, lam, vara_, vare_, vt, loop_seconds).c_str());
}

// posterior assembly, src/Bayes.cpp:919-1040
int hb_run::finish(hb_bayes_out *o)
{
    int rc;
    HB_HIP(hipSetDevice(c->device));
    const double Rn = (double)n_records;
    o->n_records = n_records;
    o->n_levels = n_levels;
    o->nw = nw;
    o->Vg = vara_sum / Rn;
    o->Ve = vare_sum / Rn;
    o->h2 = hsq_sum / Rn;
    const double Mu = mu_sum / Rn;
    o->mu = Mu;
    std::vector<double> e(n), nz(m), asum(m), asq(m);
    for (int i = 0; i < n; i++) e[i] = y[i] - Mu;
    for (int i = 0; i < nc; i++) {
        const double b = beta_sum[i] / Rn;
        if (o->beta) o->beta[i] = b;
        const double *ci = Cmat.data() + (size_t)i * n;
        for (int k = 0; k < n; k++) e[k] -= b * ci[k];
    }
    rc = hb_ctx_get_counters(c, nz.data(), asum.data(), asq.data());
    if (rc) return rc;
    for (int i = 0; i < m; i++) {
        const double mean = asum[i] / Rn;
        if (o->alpha_sd) o->alpha_sd[i] = n_records > 1 ? std::sqrt(std::max(0.0, (asq[i] - Rn * mean * mean) / (Rn - 1))) : 0.0;
        asum[i] = mean;
    }
    if (poly) { // :955-964: the polygenic vector's back-projection onto the markers joins alpha and every stored alpha column
        if (!poly_finished) {
            std::vector<double> v(n), r_keep(n);
            k_mean.assign(n, 0.0);
            ghat.assign(m, 0.0);
            rc = hbk_poly_backproject(c, sumvx, count, k_mean.data(), v.data());
            if (rc) return rc;
            // X'v through the panel mat-vec with v in the residual's place (the chain is over; the residual is put back)
            rc = hb_ctx_get_residual(c, r_keep.data(), nullptr);
            if (!rc) rc = hb_ctx_set_residual(c, v.data(), nullptr);
            if (!rc) rc = hb_ctx_dot(c, 0, m, ghat.data());
            if (!rc) rc = hb_ctx_set_residual(c, r_keep.data(), nullptr);
            if (rc) return rc;
            const double gm = arma_sum(ghat.data(), ghat.size()) / (double)m;
            for (double &gv : ghat) gv -= gm;
            for (size_t rr = 0; rr < s_alpha.size() / (size_t)m; rr++)
                for (int i = 0; i < m; i++) s_alpha[rr * m + i] += ghat[i];
            poly_finished = true;
        }
        for (int i = 0; i < m; i++) asum[i] += ghat[i];
    }
    if (o->alpha) std::memcpy(o->alpha, asum.data(), sizeof(double) * m);
    { // e -= X * alpha (:971): one device mat-vec; shards sum their partial products
        std::vector<double> xa(n);
        rc = hb_ctx_matvec(c, asum.data(), xa.data());
        if (rc) return rc;
        if (sharded) {
            rc = allreduce_host(xa.data(), n);
            if (rc) return rc;
        }
        for (int k = 0; k < n; k++) e[k] -= xa[k];
    }
    { // the state after the last iteration (hb_bayes_out.last), before Pi becomes its posterior mean below
        o->last = hb_warm_state{};
        o->last.mu = mu;
        o->last.vare = vare_;
        o->last.varg = varg;
        o->last.lambda2 = lambda2;
        for (int j = 0; j < n_fold; j++) o->last.pi[cls_of[j]] = Pi[j];
        o->last.vargL = o->vargL_last;
        if (o->g_last || o->vargL_last) {
            rc = hb_ctx_get_effects(c, o->g_last, nullptr, o->vargL_last);
            if (rc) return rc;
        }
    }
    if (!fixpi) {
        for (int j = 0; j < n_fold; j++) Pi[j] = pi_sum[j] / Rn;
    } else { // :979-983
        for (int r = 0; r < n_records; r++) {
            s_pi[(size_t)r * n_fold + 0] = Pi[0];
            s_pi[(size_t)r * n_fold + 1] = Pi[1];
        }
    }
    if (o->pi) for (int j = 0; j < n_pi; j++) o->pi[cls_of[j]] = Pi[j]; // (the caller's class order)
    if (nr) {
        for (int t = 0; t < nr; t++) {
            if (o->Vr) o->Vr[t] = vr_sum[t] / Rn;
            if (o->r_term_nlevels) o->r_term_nlevels[t] = nlev[t];
        }
        std::vector<double> est(n_levels);
        for (int q = 0; q < n_levels; q++) est[q] = estR_sum[q] / Rn;
        for (int t = 0; t < nr; t++)
            for (int k = 0; k < n; k++) e[k] -= est[lev_first[t] + zid[(size_t)t * n + k]];
        if (o->r_est) std::memcpy(o->r_est, est.data(), sizeof(double) * n_levels);
    }
    if (epsl) { // :987-994: e -= mean(J) y_J, e.tail(ne) -= Z mean(epsilon)
        if (!epsl_finished) {
            eps_mean.assign(qe, 0.0);
            std::vector<int32_t> idx(ne);
            rc = hbk_epsl_sum(c, eps_mean.data(), idx.data());
            if (rc) return rc;
            for (double &v : eps_mean) v /= Rn;
            eps_index.resize(ne);
            for (int r = 0; r < ne; r++) eps_index[r] = (uint32_t)idx[r];
            epsl_finished = true;
        }
        const double Jm = n_records > 0 ? arma_sum(s_J.data(), s_J.size()) / Rn : 0.0;
        for (int k = 0; k < n; k++) e[k] -= Jm * eps_yJ[k];
        for (int r = 0; r < ne; r++) e[n - ne + r] -= eps_mean[eps_index[r]];
    }
    if (o->g) { rc = hb_ctx_get_residual(c, nullptr, o->g); if (rc) return rc; } // :1023, final-iteration u
    if (o->e) std::memcpy(o->e, e.data(), sizeof(double) * n);
    if (o->pip) {
        if (always_in) for (int i = 0; i < m; i++) o->pip[i] = 1.0; // :1026-1027
        else for (int i = 0; i < m; i++) o->pip[i] = hb_pip(nz[i], nzct); // :1030
    }
    if (nw && o->gwas) { // :1034-1038; windows must not straddle shards (hibayes_amd/dist.py checks)
        std::vector<double> w(nw);
        rc = hb_ctx_get_windows(c, w.data());
        if (rc) return rc;
        if (sharded) { // (chunked: the exchange buffer holds n + 16 values)
            rc = allreduce_chunks(w.data(), w.size());
            if (rc) return rc;
        }
        for (int k = 0; k < nw; k++) o->gwas[k] = hb_pip(w[k], nzct);
    }
    o->nzct = nzct;
    auto cp = [](double *dst, const std::vector<double> &src) { if (dst && !src.empty()) std::memcpy(dst, src.data(), sizeof(double) * src.size()); };
    cp(o->s_mu, s_mu); cp(o->s_Vg, s_Vg); cp(o->s_Ve, s_Ve); cp(o->s_h2, s_h2);
    if (o->s_pi)
        for (int r = 0; r < n_records; r++)
            for (int j = 0; j < n_fold; j++) o->s_pi[(size_t)r * n_fold + cls_of[j]] = s_pi[(size_t)r * n_fold + j];
    cp(o->s_beta, s_beta); cp(o->s_Vr, s_Vr); cp(o->s_r, s_r);
    if (a.store_alpha) cp(o->s_alpha, s_alpha);
    o->setup_seconds = setup_seconds;
    o->loop_seconds = loop_seconds;
    o->iters_done = iter;
    o->mean_events = iter > 0 ? events_sum / iter : 0;
    o->sweeps_replayed = replay.aborts;
    o->resident_bits = c ? c->layout : 0;
    line("Posterior parameters:");
    line("    Mu %f", Mu);
    line("    Genetic var %f", o->Vg);
    line("    Residual var %f", o->Ve);
    line("    Estimated h2 %f", o->h2);
    line("Finished: set-up %.2fs (Gram %.2fs), MCMC %.2fs, %.1f sweeps/s", setup_seconds, gram_seconds, loop_seconds,
         loop_seconds > 0 ? iter / loop_seconds : 0.0);
    return HB_OK;
}

extern "C" {

int hb_run_create(const hb_bayes_args *args, hb_run **out)
{
    if (!args || !out) return hb_fail(HB_ERR_INVALID, "hb_run_create: null argument");
    *out = nullptr;
    hb_run *r = new hb_run();
    const int rc = r->setup(args);
    if (rc) {
        delete r;
        return rc;
    }
    *out = r;
    return HB_OK;
}

int hb_run_step(hb_run *r, int32_t nsteps, int32_t *finished)
{
    if (!r) return hb_fail(HB_ERR_INVALID, "hb_run_step: null run");
    for (int s = 0; s < nsteps && !r->done; s++) {
        const int rc = r->step();
        if (rc) return rc;
    }
    if (finished) *finished = r->done ? 1 : 0;
    return HB_OK;
}

int hb_run_state(hb_run *r, hb_run_info *info)
{
    if (!r || !info) return hb_fail(HB_ERR_INVALID, "hb_run_state: null argument");
    info->iter = r->iter;
    info->records = r->count;
    info->nnz = (double)r->NnzSnp;
    info->vara = r->vara_;
    info->vare = r->vare_;
    info->varg = r->varg;
    info->mu = r->mu;
    for (int j = 0; j < HB_MAX_FOLD; j++) info->pi[j] = 0.0;
    for (int j = 0; j < r->n_fold; j++) info->pi[r->cls_of[j]] = r->Pi[j];
    info->mean_events = r->iter > 0 ? r->events_sum / r->iter : 0.0;
    info->mean_misses = r->iter > 0 ? r->miss_sum / r->iter : 0.0;
    info->mean_redo = r->iter > 0 ? r->redo_sum / r->iter : 0.0;
    info->sweeps_replayed = r->replay.aborts;
    info->resident_bits = r->c ? r->c->layout : 0;
    info->lambda2 = r->lambda2;
    info->loop_seconds = r->loop_seconds;
    info->setup_seconds = r->setup_seconds;
    info->gram_seconds = r->gram_seconds;
    return HB_OK;
}

hb_ctx *hb_run_ctx(hb_run *r) { return r ? r->c : nullptr; }

int hb_run_poly(hb_run *r, hb_poly_out *po)
{
    if (!r || !po) return hb_fail(HB_ERR_INVALID, "hb_run_poly: null argument");
    if (!r->poly) return hb_fail(HB_ERR_INVALID, "hb_run_poly: the run has no polygenic block (model \"BSLMM\" with Kival / Ki)");
    if (!r->poly_finished) return hb_fail(HB_ERR_INVALID, "hb_run_poly: call hb_run_finish first");
    const int R = r->n_records;
    auto mean_sd = [&](const std::vector<double> &v, double *mean, double *sd) { // arma::mean / stddev (N - 1), :965-968
        *mean = R > 0 ? arma_sum(v.data(), v.size()) / R : 0.0;
        *sd = std::sqrt(var_n1(v.data(), v.size()));
    };
    mean_sd(r->s_Va, &po->Va, &po->Va_sd);
    mean_sd(r->s_Vb, &po->Vb, &po->Vb_sd);
    if (po->s_Va && R) std::memcpy(po->s_Va, r->s_Va.data(), sizeof(double) * R);
    if (po->s_Vb && R) std::memcpy(po->s_Vb, r->s_Vb.data(), sizeof(double) * R);
    if (po->k_mean) std::memcpy(po->k_mean, r->k_mean.data(), sizeof(double) * r->n);
    if (po->ghat) std::memcpy(po->ghat, r->ghat.data(), sizeof(double) * r->m);
    return HB_OK;
}

int hb_run_epsl(hb_run *r, hb_epsl_out *eo)
{
    if (!r || !eo) return hb_fail(HB_ERR_INVALID, "hb_run_epsl: null argument");
    if (!r->epsl) return hb_fail(HB_ERR_INVALID, "hb_run_epsl: the run has no epsilon block (epsl_y_J / epsl_Gi / epsl_index)");
    if (!r->epsl_finished) return hb_fail(HB_ERR_INVALID, "hb_run_epsl: call hb_run_finish first");
    const int R = r->n_records;
    auto mean_sd = [&](const std::vector<double> &v, double *mean, double *sd) { // arma::mean / stddev (N - 1), :988-991
        *mean = R > 0 ? arma_sum(v.data(), v.size()) / R : 0.0;
        *sd = std::sqrt(var_n1(v.data(), v.size()));
    };
    mean_sd(r->s_Veps, &eo->Veps, &eo->Veps_sd);
    mean_sd(r->s_J, &eo->J, &eo->J_sd);
    if (eo->s_Veps && R) std::memcpy(eo->s_Veps, r->s_Veps.data(), sizeof(double) * R);
    if (eo->s_J && R) std::memcpy(eo->s_J, r->s_J.data(), sizeof(double) * R);
    if (eo->epsilon) std::memcpy(eo->epsilon, r->eps_mean.data(), sizeof(double) * r->qe);
    if (eo->s_epsilon) {
        if (!r->store_eps) return hb_fail(HB_ERR_INVALID, "hb_run_epsl: the run kept no epsilon records (hb_run_epsl_store(r, 0))");
        if (R) std::memcpy(eo->s_epsilon, r->s_eps.data(), sizeof(double) * (size_t)R * r->qe);
    }
    return HB_OK;
}

int hb_run_epsl_store(hb_run *r, int32_t store_epsilon)
{
    if (!r) return hb_fail(HB_ERR_INVALID, "hb_run_epsl_store: null run");
    if (!r->epsl) return hb_fail(HB_ERR_INVALID, "hb_run_epsl_store: the run has no epsilon block (epsl_y_J / epsl_Gi / epsl_index)");
    if (r->iter > 0) return hb_fail(HB_ERR_INVALID, "hb_run_epsl_store: the run has started");
    r->store_eps = store_epsilon != 0;
    if (r->store_eps) r->s_eps.assign((size_t)r->n_records * r->qe, 0.0);
    else std::vector<double>().swap(r->s_eps);
    return HB_OK;
}

int hb_run_finish(hb_run *r, hb_bayes_out *out)
{
    if (!r || !out) return hb_fail(HB_ERR_INVALID, "hb_run_finish: null argument");
    return r->finish(out);
}

void hb_run_destroy(hb_run *r) { delete r; }

int hb_bayes_run(const hb_bayes_args *args, hb_bayes_out *out) { return hb_bayes_run_poly(args, out, nullptr); }

int hb_bayes_run_poly(const hb_bayes_args *args, hb_bayes_out *out, hb_poly_out *poly_out) { return hb_bayes_run_epsl(args, out, poly_out, nullptr); }

int hb_bayes_run_epsl(const hb_bayes_args *args, hb_bayes_out *out, hb_poly_out *poly_out, hb_epsl_out *epsl_out)
{
    if (!args || !out) return hb_fail(HB_ERR_INVALID, "hb_bayes_run: null argument");
    hb_run *r = nullptr;
    int rc = hb_run_create(args, &r);
    if (rc) return rc;
    if (r->epsl && !(epsl_out && epsl_out->s_epsilon)) rc = hb_run_epsl_store(r, 0);
    while (!rc && !r->done) rc = r->step();
    if (!rc) rc = r->finish(out);
    if (!rc && poly_out) rc = hb_run_poly(r, poly_out);
    if (!rc && epsl_out) rc = hb_run_epsl(r, epsl_out);
    delete r;
    return rc;
}

} // extern "C"
