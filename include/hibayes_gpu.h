/*
 * hibayes_gpu.h — C ABI of libhibayes_gpu.so, the MI355X (gfx950) engine for hibayes'
 * individual-level per-SNP Gibbs sampler.
 *
 * Drop-in boundary.  The reference reaches this path through ONE symbol:
 *     SEXP _hibayes_Bayes(SEXP x 27)          reference src/RcppExports.cpp:16-50
 * generated from `Rcpp::List Bayes(arma::vec& y, arma::mat& X, std::string model, ...)`
 * at reference src/Bayes.cpp:60-88 and called from R/RcppExports.R:4-6 by ibrm()
 * (R/bayes.r:293-296).  hb_bayes_run() below takes that argument list one-for-one
 * (plain pointers and sizes; Nullable<T> -> pointer-or-NULL / has_* flags) and returns
 * the fields of the Rcpp::List built at src/Bayes.cpp:919-1040.  The Rcpp shim a
 * maintainer adds on the reference side is shown in INTEGRATION.md.
 *
 * All functions return 0 on success and a non-zero hb_status otherwise; the message for
 * the calling thread's last failure is hb_last_error().  Validation failures carry the
 * reference's own exception texts (src/Bayes.cpp:92-117, :293, :325, :357).  Nothing in
 * this library aborts the process, and nothing here falls back to a CPU implementation:
 * without a HIP device every compute entry point fails with HB_ERR_NO_DEVICE.
 */
#ifndef HIBAYES_GPU_H
#define HIBAYES_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HB_ABI_VERSION 6
#define HB_MAX_FOLD 8

typedef enum {
    HB_OK = 0,
    HB_ERR_INVALID = 1,     /* argument validation (reference exception text in hb_last_error) */
    HB_ERR_NO_DEVICE = 2,   /* no usable HIP device / runtime */
    HB_ERR_HIP = 3,         /* a HIP call or kernel failed */
    HB_ERR_UNSUPPORTED = 4, /* argument outside the GPU path (BSLMM without Kival / Ki, or sharded / warm; epsilon block; non-integer X on the integer
                             * layouts — genotype_bits 8 or 2, hb_ctx_upload_genotype_f64; shard_rows, marker shards, BSLMM, hb_ldm_build and
                             * hb_grm_build on the fp64 resident layout) */
    HB_ERR_COMM = 5,        /* the multi-GPU all-reduce callback failed */
    HB_ERR_INTERRUPT = 6,   /* interrupt callback asked to stop */
    HB_ERR_ABORTED = 7      /* a wait inside the device pipeline timed out and the sweep was abandoned (hb_ctx_sweep_end); the
                               sampler (hb_bayes_run / hb_run_step) restores the state it saved before the sweep and replays
                               it — the draws are counter-based, so the replay is the same chain — and only fails with this
                               status when the replays time out as well */
} hb_status;

int hb_abi_version(void);
const char *hb_version(void);
const char *hb_last_error(void);
/* number of visible HIP devices (0 when there is none; never fails) */
int hb_device_count(void);

/* ------------------------------------------------------------------------------------
 * Multi-GPU exchange.  Markers are sharded over `world` processes (one per GPU); once per
 * sweep every rank contributes a vector of `count` doubles living in DEVICE memory and
 * needs the element-wise sum over ranks back in place.  The host process supplies the
 * collective (torch.distributed / RCCL all_reduce in hibayes_amd/dist.py); the library
 * enqueues its kernels on `hip_stream` and calls this with that stream quiesced.
 * Return 0 on success.
 * ------------------------------------------------------------------------------------ */
typedef int (*hb_allreduce_fn)(void *device_buf, size_t count, void *user);
/* The same collective INSIDE the library: an RCCL communicator (librccl is dlopen()ed on first use). With
 * hb_bayes_args.comm set, the per-sweep exchange is one ncclAllReduce enqueued on the sweep's HIP stream — no host
 * synchronisation and no callback, so it also works from the R shim. Rank 0 calls hb_comm_unique_id(), ships the
 * HB_COMM_ID_BYTES to the other ranks by any means (torch.distributed / MPI / a file), every rank calls hb_comm_init(). */
#define HB_COMM_ID_BYTES 128
typedef struct hb_comm hb_comm;
int hb_comm_unique_id(void *id_out /* HB_COMM_ID_BYTES */);
int hb_comm_init(hb_comm **out, const void *id, int32_t rank, int32_t world, int32_t device);
int hb_comm_world(const hb_comm *c);   /* ranks RCCL reports for the communicator */
int hb_comm_rank(const hb_comm *c);
int hb_comm_selftest(hb_comm *c);     /* one 16-double all-reduce with a known answer, synchronised (run it under a deadline) */
void hb_comm_destroy(hb_comm *c);
typedef struct hb_ctx hb_ctx; /* device context of one genotype shard, see the engine API below */
/* called once per iteration from the calling thread; non-zero return stops the run
 * (the shim wires it to R_CheckUserInterrupt; the reference cannot be interrupted) */
typedef int (*hb_interrupt_fn)(void *user);
/* console lines the reference prints through Rcpp::Rcout (src/Bayes.cpp:393-461, :884-914,
 * :1042-1091); NULL = print to stdout when verbose */
typedef void (*hb_log_fn)(const char *line, void *user);

/* The scalars (and BayesL's per-marker variances) the loop at src/Bayes.cpp:477 carries from one iteration to the next, beside the
 * effects g: what hb_run_state() reports after an iteration is what a second run needs — together with g_init = the effects — to go
 * on in the same regime (same markers in the model, same pi / marker variance / residual variance) rather than re-admit markers from
 * the prior defaults for its first sweeps. The prior's own constants (s2varg_, dfvara_, s2vare_, rate0 ...: :319-374) are still
 * derived from the arguments exactly as in a cold run. Draws are addressed by (seed, iteration, marker) from iteration 0 of the
 * new run. bench.py's side legs and the stationary-state parity tests (tests/test_gpu_configs.py) start runs this way; the oracle
 * takes the same state (hbo_args.warm). */
typedef struct hb_warm_state {
    double mu;               /* intercept (:469)                                           */
    double vare;             /* residual variance vare_ (:823)                             */
    double varg;             /* shared marker variance (RR / C / R: :603, :713, :807); ignored by A / B / L */
    double lambda2;          /* BayesL (:738-741); ignored elsewhere                       */
    double pi[HB_MAX_FOLD];  /* class proportions in the CALLER's class order (as hb_run_info.pi); used unless the model fixes pi
                                (BayesB / BayesC, :669 / :716) or has none (RR / A / L)   */
    const double *vargL;     /* BayesL: m per-marker variances (:730), NULL = the prior's fill (:364-368) */
} hb_warm_state;

/* ------------------------------------------------------------------------------------
 * Arguments of Bayes(), reference src/Bayes.cpp:60-88, same order.
 * ------------------------------------------------------------------------------------ */
typedef struct hb_bayes_args {
    int32_t n;               /* y.n_elem == X.n_rows                                       */
    int32_t m;               /* X.n_cols (LOCAL columns when sharded)                      */
    const double *y;         /* arma::vec& y                                        (:61) */
    /* arma::mat& X (:62).  Exactly one of the two must be non-NULL.  X_f64 is the
     * reference's layout (column-major doubles) and must hold integers in [-127,127]
     * (0/1/2 or -1/0/1 genotype codes); X_i8 is the fast path that skips the double
     * blow-up (e.g. the bigmemory .bin mapping, R/read_plink.r:57-65).                     */
    const double *X_f64;
    int64_t ld_f64;          /* leading dimension in elements (>= n)                       */
    const int8_t *X_i8;
    int64_t ld_i8;
    const char *model;       /* std::string model                                    (:63) */
    const double *Pi;        /* arma::vec Pi                                         (:64) */
    int32_t n_pi;
    const double *Kival;     /* BSLMM only (:65): the n eigenvalues of the relationship matrix (make_grm(eigen = TRUE), R/bayes.r:292-294) */
    const double *Ki;        /* BSLMM only (:66): its n x n eigenvectors, column-major, leading dimension n. Both or neither; with another
                                model, or model "BSLMM" without them (and without a ctx prepared by hb_ctx_poly_setup): HB_ERR_UNSUPPORTED */
    const double *C;         /* Nullable<arma::mat> C, n x nc column-major           (:67) */
    int32_t nc;
    const char *const *R;    /* Nullable<CharacterMatrix> R, n x nr column-major      (:68) */
    int32_t nr;
    const double *fold;      /* Nullable<arma::vec> fold                             (:69) */
    int32_t n_fold;
    int32_t niter;           /* (:70) default 50000 */
    int32_t nburn;           /* (:71) default 20000 */
    int32_t thin;            /* (:72) default 5     */
    const double *epsl_y_J;  /* single-step epsilon block (:73-75, :554-584): all three or none. epsl_y_J: the n values of the J covariate */
    const void *epsl_Gi;     /* -> hb_epsl_gi (below): the q x q matrix of the non-genotyped individuals, A^-1_nn, and ne                 */
    const uint32_t *epsl_index; /* ne entries, 1-BASED as the reference takes them (:255-256): the column of epsl_Gi of each of the LAST ne
                                records. With marker shards, shard_rows, a warm start or BSLMM: HB_ERR_UNSUPPORTED                        */
    /* Nullable<double> dfvr..s2ve (:76-83): value used only when the has_ flag is set      */
    int32_t has_dfvr, has_s2vr, has_vg, has_dfvg, has_s2vg, has_ve, has_dfve, has_s2ve;
    double dfvr, s2vr, vg, dfvg, s2vg, ve, dfve, s2ve;
    const uint32_t *windindx; /* Nullable<arma::uvec> windindx, m, 1-based           (:84) */
    int32_t outfreq;          /* (:85) */
    int32_t threads;          /* (:86) accepted and ignored: there is no OpenMP region     */
    int32_t verbose;          /* (:87) */

    /* ---- additions that have no reference counterpart ---- */
    uint64_t seed;            /* replaces R's global RNG state (set.seed(), R/bayes.r:151)  */
    int32_t device;           /* HIP device ordinal                                         */
    int32_t panel;            /* markers per block-Gibbs panel: 0 = auto, else 64..1024     */
    int32_t precise;          /* arithmetic of the panel mat-vec x_j . yadj: 2 exact fixed point (fp64 residual as
                                 7 int8 digit planes, int8 x int8 -> int32; recommended), 1 fp64 FMA, 0 fp32 image */
    int32_t store_alpha;      /* keep MCMCsamples$alpha (m x n_records) — see hb_bayes_out  */
    /* marker sharding: this process owns global columns [m_offset, m_offset + m)           */
    int32_t rank, world;
    int64_t m_global, m_offset;
    hb_allreduce_fn allreduce;
    void *allreduce_user;
    void *exchange_buf;       /* optional caller-owned DEVICE buffer the collective runs on,
                                 >= hb_exchange_count(n) doubles (a torch tensor)            */
    hb_interrupt_fn interrupt;
    void *interrupt_user;
    hb_log_fn log;
    void *log_user;
    /* optional pre-loaded context: genotypes already resident on the device (then X_f64 and X_i8
     * must be NULL and n, m must match). Lets one upload serve several model fits.            */
    hb_ctx *ctx;
    /* warm start (no reference counterpart; ABI 2): m effects the chain starts from instead of g = 0
     * (src/Bayes.cpp:297). yadj = y - mu - X g_init, u = X g_init; classes restart as (g != 0). */
    const double *g_init;
    /* in-library RCCL collective (takes precedence over `allreduce`); with world == 1 the exchange path still runs,
     * which is how a one-GPU box exercises it */
    hb_comm *comm;
    /* the sharded sweep's `sync_every_blocks` knob (ABI 3): the shards exchange their residual deltas this many
     * times per sweep, after equal runs of mat-vec groups, instead of once at its end (0 or 1). Inside a run a shard still does
     * not see the other shards' moves; more exchanges = less of that staleness (and of the bias it causes where the shards'
     * markers are correlated), at one all-reduce and one pipeline drain each. Unsharded, the chain does not depend on it. */
    int32_t sync_blocks;
    /* resident genotype layout of the sweep (ABI 4; 0 = auto since round 6): 8 = int8 columns; 2 = 2 bits per genotype, PLINK's
     * own density (reference src/read_bed.cpp:116-167), expanded to bytes in registers inside the mat-vec — a
     * quarter of the bytes per sweep. Needs genotype codes 0..3 and the fixed-point mat-vec (precise = 2); same chain bit for bit
     * (the dot products are exact integers either way). A context the run creates drops its int8 copy once the Gram blocks
     * are built; with a pre-loaded ctx the layout is the context's (hb_ctx_set_layout).
     * 0 = AUTO (what the Rcpp shim and ibrm() pass): 2 bits where that is exact and the faster sweep — every code in 0..3, precise = 2,
     * BayesB / BayesBpi / BayesC / BayesCpi (450 against 213 sweeps/s at n = 50k, m = 500k) and BayesR with up to four classes (103 against 98
     * converged, 64.5 against 58 cold) at panel 512, the band and the packed copy fitting the device — int8 columns otherwise (the models in which
     * every marker moves, other genotype codes, small problems). hb_bayes_out.resident_bits / hb_run_info.resident_bits
     * report the choice. HB_NO_AUTO_BITS=1 in the environment keeps int8.
     * 64 = fp64 columns, for real-valued genotypes (imputed dosages; the reference's Bayes() takes any arma::mat): any finite value, a NaN or Inf is
     * HB_ERR_INVALID with "NAs are not allowed in genotype."; X_i8 is converted on the device. The mat-vec is the fp64 FMA one whatever `precise`
     * says, the sweep runs on the event-ordered per-panel kernels (pipeline 0, lag 0, one panel per mat-vec, the diagonal Gram blocks in fp64;
     * hb_ctx_pipeline_note says so), resident_bits reports 64. Under 0 (auto) an X_f64 that is integer-valued within int8's range takes the route above
     * unchanged; any other takes 64 (it used to be refused). 8 / 2 with such a matrix stay refused (HB_ERR_UNSUPPORTED): never rounded silently.
     * Not on this layout (HB_ERR_UNSUPPORTED): shard_rows, marker shards (comm / world > 1), BSLMM. */
    int32_t genotype_bits;
    /* Exact multi-GPU cross-check mode (ABI 4; SURVEY §8e "alternative rejected ... keep only as a correctness cross-check mode"):
     * shard the INDIVIDUALS instead of the markers. This process holds rows [row_offset, row_offset + n) of all m markers and of y
     * (n_global individuals in total; row_offset and every n but the last rank's multiples of 256). The digit-plane sums of every
     * panel mat-vec are integers, so their all-reduce is exact and order-independent: every rank runs THE single-GPU chain
     * (same decisions, same effects), whatever the model — the dense models (RR / A / L) that a marker-sharded sweep biases
     * included. Price: one all-reduce per panel (through `allreduce` / `comm`, with a host round trip: the per-panel kernels, no
     * pipeline), so it scales capacity, not throughput. Needs precise = 2; covariates / random effects are refused here. */
    int32_t shard_rows;
    int64_t n_global, row_offset;
    /* Warm hyper-parameter state (ABI 6; no reference counterpart): with g_init, the state a chain is CONTINUED from instead of
     * started at the prior defaults of src/Bayes.cpp:319-374. NULL = the reference's start. See hb_warm_state above. */
    const hb_warm_state *warm;
} hb_bayes_args;


/* number of doubles exchanged per sweep for n individuals: the residual delta (u moves by its negative) + 16 scalar sums */
size_t hb_exchange_count(int32_t n);

/* ------------------------------------------------------------------------------------
 * Result, reference src/Bayes.cpp:919-1040.  Arrays are caller-allocated; a NULL pointer
 * means "not wanted".  R = n_records = (niter - nburn) / thin.
 * ------------------------------------------------------------------------------------ */
typedef struct hb_bayes_out {
    double Vg, Ve, h2, mu;   /* results["Vg"], ["Ve"], ["h2"], ["mu"]          (:934-944) */
    int32_t n_records;
    int32_t nzct;
    int32_t nw;              /* number of GWAS windows = max(windindx)                     */
    int32_t n_levels;        /* total random-effect levels                                 */
    double *beta;            /* nc                                              (:951)    */
    double *alpha;           /* m                                               (:972)    */
    double *pi;              /* n_pi                                            (:984)    */
    double *Vr;              /* nr                                              (:925)    */
    double *r_est;           /* n_levels, results["r"]$Estimation              (:1020)    */
    int32_t *r_term_nlevels; /* nr: levels per term; level names are the sorted unique
                                strings of each R column (makeZ, :36-37)                   */
    double *g;               /* n: FINAL-iteration u, not a mean               (:1023)    */
    double *e;               /* n                                              (:1024)    */
    double *pip;             /* m                                              (:1032)    */
    double *gwas;            /* nw                                             (:1037)    */
    /* MCMCsamples: */
    double *s_Vg, *s_Ve, *s_h2, *s_mu;   /* 1 x R each                         (:937-945) */
    double *s_beta;          /* nc x R col-major                                (:952)    */
    double *s_alpha;         /* m x R col-major, only when args.store_alpha     (:973)    */
    double *s_pi;            /* n_pi x R                                        (:985)    */
    double *s_Vr;            /* nr x R                                          (:926)    */
    double *s_r;             /* n_levels x R                                    (:1021)   */
    /* extras: posterior SD of alpha from the running second moment (m), timings */
    double *alpha_sd;
    double setup_seconds;    /* upload + marker statistics + Gram precompute              */
    double loop_seconds;     /* the MCMC loop only                                        */
    int32_t iters_done;
    double mean_events;      /* mean number of markers whose effect changed per sweep     */
    int32_t sweeps_replayed; /* (ABI 5) sweeps that timed out on the device and were replayed from the saved state */
    int32_t resident_bits;   /* (was reserved_) the genotype layout the sweep read: 8, 2 or 64 — what genotype_bits = 0 ("auto") chose */
    /* (ABI 6) the chain's state after its LAST iteration — what hb_bayes_args.g_init / .warm of a following run take to continue it:
     * the scalars in `last` (last.vargL is set to vargL_last), the effects in g_last (m, caller-allocated or NULL) and, for BayesL,
     * the per-marker variances in vargL_last (m, caller-allocated or NULL). */
    hb_warm_state last;
    double *g_last;
    double *vargL_last;
} hb_bayes_out;

/* The whole sampler: replaces Bayes() (reference src/Bayes.cpp:60-1094). */
int hb_bayes_run(const hb_bayes_args *args, hb_bayes_out *out);

/* BSLMM (src/Bayes.cpp:518-552, :854-858, :955-969): what the polygenic block adds to the result. The reference only prints Va / Vb
 * (:901, :1074); the records, the mean polygenic vector and the back-projection are extensions. Caller-allocated arrays, NULL = not wanted. */
typedef struct hb_poly_out {
    double Va, Vb, Va_sd, Vb_sd; /* mean and sd (N - 1) of the records (:965-968) */
    double *s_Va, *s_Vb;     /* R each: va = varg (:715) and vb (:550) at the thinned records (:855-856) */
    double *k_mean;          /* n: k_estR_store / count (:956) */
    double *ghat;            /* m: X'(K ((K' k_mean) / Kval / sumvx)), centred (:957-962); already added to alpha and to every s_alpha column (:964) */
} hb_poly_out;
/* hb_bayes_run that also reports the polygenic block; hb_bayes_run(args, out) is hb_bayes_run_poly(args, out, NULL). poly_out with a run
 * that has no polygenic block is HB_ERR_INVALID. */
int hb_bayes_run_poly(const hb_bayes_args *args, hb_bayes_out *out, hb_poly_out *poly_out);

/* The single-step model (ssbrm(), R/ssbayes.r; src/Bayes.cpp:254-275, :554-584, :873-878, :987-1001). hb_bayes_args.epsl_Gi points at this
 * descriptor: the FULL symmetric q x q matrix (both triangles) in canonical compressed-sparse-column form — indptr q + 1 entries from 0,
 * the row indices of a column 0-based, sorted and unique, a positive diagonal stored in every column, finite values — and ne, the length of
 * epsl_index. Anything else is HB_ERR_INVALID. */
typedef struct hb_epsl_gi {
    int32_t q, ne;
    const int64_t *indptr;
    const int32_t *indices;
    const double *data;
} hb_epsl_gi;
/* What the epsilon block adds to the result. Caller-allocated arrays, NULL = not wanted; s_epsilon == NULL in hb_bayes_run_epsl is the
 * reference's store without the q x R matrix (store_epsilon = 0): only the running mean is kept. */
typedef struct hb_epsl_out {
    double Veps, Veps_sd, J, J_sd; /* mean and sd (N - 1) of the records (:988-991) */
    double *s_Veps, *s_J;    /* R each (:874-875) */
    double *epsilon;         /* q: the mean of the records (:992) */
    double *s_epsilon;       /* q x R column-major (:876) */
} hb_epsl_out;
/* hb_bayes_run that also reports the epsilon block (and the polygenic one: never both in one run); either out may be NULL. epsl_out with a
 * run that has no epsilon block is HB_ERR_INVALID. */
int hb_bayes_run_epsl(const hb_bayes_args *args, hb_bayes_out *out, hb_poly_out *poly_out, hb_epsl_out *epsl_out);
/* the descriptor's and the index's validation alone (no device needed): HB_OK or HB_ERR_INVALID with the reason in hb_last_error() */
int hb_epsl_check(const hb_epsl_gi *Gi, const uint32_t *epsl_index, int32_t n);
/* The schedule of the Gibbs pass for a pattern (hb_epslplan.hpp; no device needed): level[q], rows[q] (the rows in launch order), steps
 * (5 ints each: level, first lane row, lane rows, first wave row, wave rows — positions in rows[]; room for q steps), launches (3 ints
 * each: kind 0 = one workgroup walks steps [s0, s1) / 1 = step s0 over the chip, s0, s1; room for q), counts[4] = steps, launches, levels,
 * longest column. sched_mode 0 auto / 1 all single-workgroup / 2 all wide; row_mode 0 auto / 1 lanes only / 2 waves only. NULL = not wanted. */
int hb_epsl_plan(int32_t q, const int64_t *indptr, const int32_t *indices, int32_t sched_mode, int32_t row_mode, int32_t *level, int32_t *rows,
                 int32_t *steps, int32_t *launches, int32_t *counts);

/* The same sampler, stepwise: create (validation, upload, marker statistics, Gram, priors) ->
 * step (iterations of the loop at src/Bayes.cpp:477) -> finish (posterior assembly, :919-1040).
 * hb_bayes_run() is exactly create + step-until-finished + finish. The caller's arrays are copied
 * at create time. */
typedef struct hb_run hb_run;
typedef struct hb_run_info {
    int32_t iter;            /* iterations done */
    int32_t records;         /* thinned records stored */
    double nnz;              /* NumNZSnp of the last sweep */
    double vara, vare, varg, mu;
    double pi[HB_MAX_FOLD];
    double mean_events;      /* mean markers changed per sweep so far */
    double mean_misses;      /* mean row-cache misses per sweep so far */
    double mean_redo;        /* mean rolled-back chain rounds per sweep so far */
    double loop_seconds, setup_seconds, gram_seconds;
    int32_t sweeps_replayed; /* (ABI 5) sweeps whose device pipeline timed out and that were replayed from the saved state (HB_ERR_ABORTED) */
    int32_t resident_bits;   /* (was reserved_) the genotype layout the sweep read: 8, 2 or 64 — what genotype_bits = 0 ("auto") chose */
    double lambda2;          /* (ABI 6) BayesL's lambda^2 after the last iteration (hb_warm_state.lambda2) */
} hb_run_info;
int hb_run_create(const hb_bayes_args *args, hb_run **out);
int hb_run_step(hb_run *r, int32_t nsteps, int32_t *finished);
int hb_run_state(hb_run *r, hb_run_info *info);
hb_ctx *hb_run_ctx(hb_run *r);
int hb_run_finish(hb_run *r, hb_bayes_out *out);
/* after hb_run_finish of a BSLMM run: the polygenic block's results */
int hb_run_poly(hb_run *r, hb_poly_out *poly_out);
/* after hb_run_finish of a run with the epsilon block: its results */
int hb_run_epsl(hb_run *r, hb_epsl_out *epsl_out);
/* before the first step: keep the q x R matrix of epsilon records (default 1), or the running mean alone (0) */
int hb_run_epsl_store(hb_run *r, int32_t store_epsilon);
void hb_run_destroy(hb_run *r);

/* ------------------------------------------------------------------------------------
 * Summary-level sampler on a dense LD matrix: replaces SBayesD(), reference src/SBayesD.cpp:5-609, reached
 * through _hibayes_SBayesD (src/RcppExports.cpp:53, arity 18) from sbrm() (R/sbayes.r:213). Arguments in the reference's
 * order (:5-26); errors carry its exception texts (:30-63, :123-125, :154-156). The same six conditionals as Bayes() with the
 * right-hand sides kept in Gram space, r_hat += n (g_old - g_new) ldm[:, i] (:262-266): groups of 512 markers, the candidate-
 * round chain kernel with the LD matrix as its Gram matrix, a whole-chip column update per group (hb_sbayes.hpp).
 * ------------------------------------------------------------------------------------ */
typedef struct hb_sbayes_args {
    int32_t m;               /* ldm.n_rows == sumstat.n_rows                                              */
    const double *sumstat;   /* arma::mat sumstat (:6): m x 4 column-major — the columns sbrm() keeps,
                                R/sbayes.r:207: MAF, BETA, SE, NMISS; NaN = NA (the marker is then skipped, :102-104) */
    int64_t ld_sumstat;      /* leading dimension (>= m)                                                  */
    const double *ldm;       /* arma::mat ldm (:7): m x m column-major dense LD variance-covariance matrix */
    int64_t ld_ldm;
    const char *model;       /* (:8)  */
    const double *Pi;        /* (:9)  */
    int32_t n_pi;
    int32_t niter, nburn, thin; /* (:10-12) defaults 50000 / 20000 / 5 */
    const double *fold;      /* Nullable (:13) */
    int32_t n_fold;
    const uint32_t *windindx; /* Nullable (:14), m, 1-based */
    int32_t has_vg, has_dfvg, has_s2vg, has_ve, has_dfve, has_s2ve; /* Nullable<double> (:15-20) */
    double vg, dfvg, s2vg, ve, dfve, s2ve;
    int32_t outfreq, threads, verbose; /* (:21-23); threads is accepted and ignored */
    /* ---- additions without a reference counterpart ---- */
    uint64_t seed;           /* replaces R's global RNG state (set.seed(), R/sbayes.r:132) */
    int32_t device;
    int32_t store_alpha;     /* keep MCMCsamples$alpha (m x n_records) */
    hb_interrupt_fn interrupt;
    void *interrupt_user;
    hb_log_fn log;
    void *log_user;
} hb_sbayes_args;

/* Result list of SBayesD(), src/SBayesD.cpp:541-580. Caller-allocated arrays, NULL = not wanted; R = (niter - nburn) / thin. */
typedef struct hb_sbayes_out {
    double Vg, Ve, h2;
    int32_t n_records, nzct, nw;
    int32_t n;               /* population size the sampler used: mean of the finite NMISS, truncated (:33-34) */
    int32_t count_y;         /* markers with summary statistics (:111) */
    double *alpha;           /* m  (:553) */
    double *pi;              /* n_pi (:566) */
    double *pip;             /* m  (:575) */
    double *gwas;            /* nw (:580) */
    double *s_Vg, *s_Ve, *s_h2; /* 1 x R (:547-549) */
    double *s_alpha;         /* m x R column-major, only with store_alpha (:554) */
    double *s_pi;            /* n_pi x R (:567) */
    double *r_hat;           /* extras: the Gram-space right-hand side and the effects after the last sweep (m each) */
    double *g_last;
    double setup_seconds, loop_seconds;
    int32_t iters_done;
    double mean_events;
} hb_sbayes_out;

int hb_sbayes_run(const hb_sbayes_args *args, hb_sbayes_out *out);

/* ------------------------------------------------------------------------------------
 * The LD variance-covariance matrix of a context's resident genotypes: replaces ldmat(), reference R/ldm.r:31-112, i.e.
 * BigStat (src/tXXmat.cpp:43-77) and tXXmat_Geno (:100-206) / tXXmat_Chr (:504-626); the four *_gwas variants (:208-502,
 * :628-) are out of scope. The cross-products run on the matrix cores as exact integers, the reference's fp64 arithmetic
 * follows per entry in its own order (`p12 -= sum1 * m2 + sum2 * m1 - ind * m1 * m2; p12 / ind`, :145-152, with the marker of
 * the smaller index in the sum1 / m1 role): every entry equals the reference's bit for bit.
 * ------------------------------------------------------------------------------------ */
typedef struct hb_ldm hb_ldm; /* a finished LD matrix: host copy (pinned), optionally a dense device copy for the sampler */

enum {
    HB_LDM_KIND_DENSE = 0,        /* tXXmat_Geno, dense arm (:158-184): diagonal xx * xx / ind (:168)                      */
    HB_LDM_KIND_SPARSE = 1,       /* tXXmat_Geno, sparse arm (:124-157): entries with r * r * ind <= chisq dropped (:147),
                                     the diagonal through the same formula and test                                        */
    HB_LDM_KIND_BLOCK_DENSE = 2,  /* tXXmat_Chr without chisq (:565-604): nothing across chromosomes, sp_mat result        */
    HB_LDM_KIND_BLOCK_SPARSE = 3  /* tXXmat_Chr with chisq (:527-564), chisq = 0 included (:520-523)                       */
};

typedef struct hb_ldm_stats {
    int32_t m, kind;
    int32_t on_device;       /* a dense m x m device copy (leading dimension m) is held */
    int32_t n_strips;        /* column strips the build took */
    int64_t nnz;             /* stored entries (m * m for HB_LDM_KIND_DENSE) */
    double seconds;          /* the whole build */
    double stats_seconds, strip_seconds, compact_seconds, transfer_seconds; /* BigStat / cross-products and epilogue /
                                compaction to (row, value) lists / device-to-host copies */
} hb_ldm_stats;

/* chr: m chromosome ids (tXXmat_Chr's `chr`, R/ldm.r:91; markers of one id need not be contiguous, :531) or NULL for the
 * genome-wide matrix (R/ldm.r:88). has_chisq / chisq: Nullable<double> chisq. The mode follows the reference: without chr
 * sparse iff chisq > 0 (src/tXXmat.cpp:117-120), with chr sparse iff chisq is given (:520-523), block-dense otherwise.
 * strip_bytes: device staging per column strip, 0 = at most 1 GiB. The context must hold genotypes (int8 or 2-bit resident)
 * with max|x|^2 * n < 2^31, as for hb_ctx_build_gram. */
int hb_ldm_build(hb_ctx *ctx, const int32_t *chr, int32_t has_chisq, double chisq, int64_t strip_bytes, hb_ldm **out);
int hb_ldm_info(const hb_ldm *ldm, hb_ldm_stats *stats);
/* m x m column-major, zeros where a sparse or block matrix stores nothing (src/tXXmat.cpp:179, :152) */
int hb_ldm_download_dense(hb_ldm *ldm, double *out, int64_t ldo);
/* canonical CSC as arma::sp_mat / dgCMatrix holds it (src/tXXmat.cpp:152, :558, :599): indptr m + 1, indices and data nnz,
 * rows sorted inside a column, no stored zero. Not for HB_LDM_KIND_DENSE. */
int hb_ldm_download_csc(hb_ldm *ldm, int64_t *indptr, int32_t *indices, double *data);
void hb_ldm_destroy(hb_ldm *ldm);

/* hb_sbayes_run with args->ldm == NULL and the matrix taken from the handle's dense device copy (made on the device from the
 * stored entries if the build kept none): ldmat() -> sbrm() (R/ldm.r:88 -> R/sbayes.r:213) with no host matrix in between. */
int hb_sbayes_run_ldm(const hb_sbayes_args *args, hb_ldm *ldm, hb_sbayes_out *out);

/* A handle (HB_LDM_KIND_SPARSE) from a host CSC matrix, e.g. a scipy csc_matrix or a dgCMatrix: indptr m + 1, indices and data
 * indptr[m] long. Refused with HB_ERR_INVALID and a text: rows not sorted or not unique inside a column, an index outside
 * [0, m), and a matrix that does not equal its transpose in pattern and in value bits. The reference's SBayesS() does not need
 * symmetry; the sparse sweep here reads row j of the matrix as column j, and every LD matrix has it (hb_ldm_build's are
 * symmetric by construction: each pair is computed once). Stored zeros are kept and count as entries, as in a dgCMatrix. */
int hb_ldm_from_csc(int32_t m, const int64_t *indptr, const int32_t *indices, const double *data, int32_t device, hb_ldm **out);

/* SBayesS() of the reference (src/SBayesS.cpp:21-40, sbrm() on a dgCMatrix, R/sbayes.r:128, :213): the summary-level sampler
 * on a sparse LD matrix, from the handle's device CSC (any kind of handle; the genome-wide dense kind with its exact zeros
 * dropped). It is not hb_sbayes_run_ldm with zeros: every marker has its own residual variance
 * varediff[i] * vara + vare with varediff[i] = (m - nnz(column i)) / m (:131-141, :285), BayesC / BayesCpi / BayesR effects with
 * g^2 * vx > vary are redrawn, at most 101 times (:388-398, :489-499), and a move walks the stored entries of its column only.
 * Nothing m x m is allocated. args->ldm must be NULL; arguments, priors, records and results are hb_sbayes_run's. */
int hb_sbayes_run_sparse(const hb_sbayes_args *args, hb_ldm *ldm, hb_sbayes_out *out);

/* ------------------------------------------------------------------------------------
 * sbrm()'s method = "CG" (R/sbayes.r:217-229): the conjugate-gradient ridge solve (V + diag(lambda)) g = b on the LD matrix,
 * replaces conjgt_den / conjgt_spa (reference src/cg.cpp:4-129) and CG() (src/solver.cpp:54-115). Set-up, exception texts and
 * console lines are the reference's; the loop runs on the device (hb_cg.hip): an fp64 symmetric mat-vec and two vector kernels
 * per iteration, stopped by a device word the host reads once per chunk of min(outfreq, 64) iterations, so g is exactly the
 * state at the reference's `break`. Every sum is formed in one fixed order: two runs agree bit for bit. The order of summation
 * is not the reference's BLAS's, which is unpinned there too.
 * ------------------------------------------------------------------------------------ */
typedef struct hb_cg_args {
    int32_t m;               /* ldm.n_rows == sumstat.n_rows (src/cg.cpp:15, :79)                          */
    const double *sumstat;   /* m x 4 column-major: MAF, BETA, SE, NMISS (R/sbayes.r:207); NaN = NA. A NaN BETA is not
                                filtered: it propagates, as in the reference                               */
    int64_t ld_sumstat;      /* leading dimension (>= m)                                                   */
    const double *ldm;       /* hb_cg_run: m x m column-major, must equal its transpose in value bits; NULL for the handle forms */
    int64_t ld_ldm;
    const double *lambda;    /* Nullable<NumericVector> lambda (:7, :71): NULL or m values                 */
    double esp;              /* (:8) default 1e-6 */
    int32_t outfreq, verbose; /* (:9-10) */
    /* ---- additions without a reference counterpart ---- */
    int32_t device;
    hb_interrupt_fn interrupt; /* polled once per chunk of iterations */
    void *interrupt_user;
    hb_log_fn log;
    void *log_user;
} hb_cg_args;

typedef struct hb_cg_out {
    double vg, ve;           /* src/cg.cpp:52-53, :115-116 */
    int32_t n;               /* (int) mean of the finite NMISS (:13) */
    int32_t count_y;         /* markers whose SE is not NA (:35) */
    int32_t iterations;      /* passes of CG()'s loop: i + 1 at its `break`, m without one */
    int32_t converged;       /* err < esp (src/solver.cpp:109) */
    double err;              /* err of the last pass */
    double *g;               /* m, caller-allocated */
    double *err_hist;        /* m or NULL: err of pass i, zero from `iterations` on */
    double setup_seconds, loop_seconds;
} hb_cg_out;

/* conjgt_den (src/cg.cpp:68-129) on a host dense matrix. A matrix that differs from its transpose is refused with
 * HB_ERR_INVALID and a text that names the first differing pair (checked on the device, about one iteration's cost). */
int hb_cg_run(const hb_cg_args *args, hb_cg_out *out);
/* conjgt_den (src/cg.cpp:68-129) with args->ldm == NULL, on the handle's dense device copy: ldmat() -> CG with no host matrix. */
int hb_cg_run_ldm(const hb_cg_args *args, hb_ldm *ldm, hb_cg_out *out);
/* conjgt_spa (src/cg.cpp:4-65) with args->ldm == NULL, on the handle's device CSC; nothing m x m is allocated. */
int hb_cg_run_sparse(const hb_cg_args *args, hb_ldm *ldm, hb_cg_out *out);

/* ------------------------------------------------------------------------------------
 * make_grm() of the reference (src/rm.cpp:5-53) from a context's resident int8 genotypes: G = Z Z' / mean(diag(Z Z')) with Z the
 * column-centred genotypes, then diag += lambda (:37, :46). The cross-products are exact integers on the matrix cores, one fixed fp64
 * expression per entry follows, one triangle is computed and mirrored: G equals its transpose bit for bit and
 * two builds agree bit for bit. G_host: n x n column-major or NULL; G_dev: NULL, or receives a device copy (leading dimension n) that
 * the caller releases with hb_grm_free. flags: HB_GRM_RAW = the centred cross-product Z Z' itself, no scaling and no lambda.
 * All markers monomorphic (mean diagonal 0; the reference returns NaN): HB_ERR_INVALID. The n x n matrix not fitting on the device:
 * HB_ERR_HIP with "out of memory" in the text. The inverse (make_grm(inverse = TRUE)) is hb_spd_inverse on G_dev, further below; the eigen-decomposition is hb_eig_*.
 * ------------------------------------------------------------------------------------ */
#define HB_GRM_RAW 1
int hb_grm_build(hb_ctx *c, double lambda, int32_t flags, double *G_host, double **G_dev);
/* Frees hb_grm_build's G_dev. Only a device matrix that this library handed out (hb_grm_build, hb_eig_upload, hb_eig_vectors, hb_eig_tridiagonal):
 * NULL and any other pointer are left alone — memory the caller allocated itself is the caller's to free. */
void hb_grm_free(double *G_dev);

/* ------------------------------------------------------------------------------------
 * The symmetric eigen-decomposition behind make_grm(eigen = TRUE) (reference src/rm.cpp:46-52: eigen_sym_dc, LAPACK dsyevd; R/bayes.r:292-294
 * hands its output to Bayes() as Kival / Ki) with its two O(n^3) stages on the device. The caller supplies the
 * O(n^2) stage between them — the eigenvalues and eigenvectors Z of the tridiagonal matrix (d, e), LAPACK dstemr or dstedc on the host:
 *     hb_eig_reduce  ->  (w, Z) = dstemr(d, e)  ->  hb_eig_vectors(Z)  ->  K = Q Z on the device, for hb_ctx_poly_setup(on_device = 1)
 * — or leaves that stage on the device too (hb_eig_tridiagonal: divide and conquer, the dstedc inside the dsyevd of src/rm.cpp:46-52), and
 * then no n x n matrix crosses the bus:
 *     hb_eig_reduce  ->  hb_eig_tridiagonal(d, e) -> (w, Z_dev)  ->  hb_eig_vectors_dev(Z_dev)  ->  K = Q Z in Z's buffer.
 * No floating-point atomics: two runs on the same matrix agree bit for bit. Without a device every entry below that computes or copies
 * fails with HB_ERR_NO_DEVICE.
 * ------------------------------------------------------------------------------------ */
typedef struct hb_eig hb_eig;
/* A host matrix (n x n column-major, leading dimension lda_host) on the device, with an even leading dimension *lda; hb_eig_release frees it.
 * hb_grm_build's G_dev needs no upload (src/rm.cpp:46: the matrix eigen_sym_dc receives). */
int hb_eig_upload(const double *A_host, int64_t lda_host, int32_t n, int32_t device, double **A_dev, int64_t *lda);
/* LAPACK dsytrd, uplo = 'L' (first stage of the dsyevd of src/rm.cpp:46-52): Q' A Q = T. Only the lower triangle of A_dev is read. A_dev is
 * overwritten as dsytrd leaves it (reflector k below the subdiagonal of column k, v[0] = 1 implied, beta = -sign(alpha) ||x||, tau = 0 for a
 * column that is exactly zero there; d on the diagonal, e on the subdiagonal) and is BORROWED until hb_eig_destroy. d_host (n) and e_host
 * (n - 1) receive the tridiagonal matrix. lda < n or n < 1: HB_ERR_INVALID; a non-finite d or e: HB_ERR_INVALID, "the matrix holds a
 * non-finite value". A 16-byte aligned A_dev with an even lda takes the fast mat-vec. */
int hb_eig_reduce(double *A_dev, int64_t lda, int32_t n, int32_t device, double *d_host, double *e_host, hb_eig **out);
/* dsytrd's TAU (n - 1 values) — with the reduced A_dev (hb_eig_download) the whole of Q; for the tests (src/rm.cpp:46-52). */
int hb_eig_tau(hb_eig *h, double *tau_host);
/* LAPACK dormtr (side L, uplo L, no transpose; last stage of the dsyevd of src/rm.cpp:46-52): *K_dev = Q Z, the matrix R/bayes.r:292-294
 * passes on as Ki. Z_host: n x n column-major with leading dimension ldz, or NULL for Z = I (K = Q, dorgtr). K is allocated here with an
 * even leading dimension *ldk (every column 16-byte aligned, as hb_ctx_poly_setup(on_device = 1) requires), is the caller's and outlives
 * the handle; hb_eig_release frees it. */
int hb_eig_vectors(hb_eig *h, const double *Z_host, int64_t ldz, double **K_dev, int64_t *ldk);
/* LAPACK dstedc (compz = 'I') on the device: the eigenvalues w_host (n, ascending) and eigenvectors Z of the symmetric tridiagonal matrix with
 * diagonal d_host (n) and off-diagonal e_host (n - 1; may be NULL for n = 1), by Cuppen's divide and conquer with Gu-Eisenstat vectors
 * (DESIGN.md section 16). Column j of *Z_dev belongs to w_host[j]; Z has hb_eig_vectors' layout — leading dimension *ldz = n rounded up to 64,
 * that many columns allocated, padding zero — is the caller's, and is freed with hb_eig_release or handed to hb_eig_vectors_dev. Refused
 * before any device is asked for, HB_ERR_INVALID: a null pointer, n < 1, a non-finite d or e. A secular iteration or a leaf that does not
 * converge within its hard cap of steps is HB_ERR_HIP with a text, never a silent result. Deterministic: no floating-point atomics. */
int hb_eig_tridiagonal(const double *d_host, const double *e_host, int32_t n, int32_t device, double *w_host, double **Z_dev, int64_t *ldz);
/* hb_eig_vectors for a Z that lies on the device (hb_eig_tridiagonal's): K = Q Z in place in Z's buffer, by the same panels. Ownership of the
 * buffer passes to *K_dev (hb_eig_release); on failure it stays the caller's. ldz other than n rounded up to 64: HB_ERR_INVALID. */
int hb_eig_vectors_dev(hb_eig *h, double *Z_dev, int64_t ldz, double **K_dev, int64_t *ldk);
/* The merge tree hb_eig_tridiagonal uses for n rows and the given split points (ascending indices i whose e_i is negligible), a pure function
 * of its arguments that needs no device: leaves [leaf_lo, leaf_hi) of at most *leaf_rows rows, merges of [lo, mid) with [mid, hi) at level
 * merge_level (children before parents; all merges of a level are disjoint and go in the same launches), *levels the highest level. cap: the
 * length of every array; n entries always suffice. */
int hb_stedc_plan(int32_t n, const int32_t *splits, int32_t nsplit, int32_t cap, int32_t *leaf_lo, int32_t *leaf_hi, int32_t *nleaf, int32_t *merge_lo,
                  int32_t *merge_mid, int32_t *merge_hi, int32_t *merge_level, int32_t *nmerge, int32_t *levels, int32_t *leaf_rows);
/* Seconds of this process's last hb_eig_tridiagonal by phase, for tools/eig_timing.py: [0] leaves (with set-up), [1] gather and deflation scan,
 * [2] rotations, secular equation and vector work, [3] U strips and GEMM, [4] copies and ordering; [5] the GEMM's floating-point operations. */
int hb_stedc_stats(double *out, int32_t count);
/* An n x n device matrix of this interface — K (the Ki of R/bayes.r:292-294), or the reduced A (src/rm.cpp:46-52) — to a host column-major array. */
int hb_eig_download(const double *M_dev, int64_t ld_dev, int32_t n, int32_t device, double *M_host, int64_t ld_host);
/* Frees what hb_eig_upload, hb_eig_vectors or hb_eig_tridiagonal allocated (the Ki of R/bayes.r:292-294 once the fit is done), or hb_grm_build's
 * G_dev. Only those: NULL and a pointer this library did not hand out are left alone — memory the caller allocated itself is the caller's to free. */
void hb_eig_release(double *M_dev);
/* Ends the borrowing of A_dev and frees the handle's panels (src/rm.cpp:46-52 keeps nothing either). NULL is allowed. */
void hb_eig_destroy(hb_eig *h);

/* ------------------------------------------------------------------------------------
 * The inverse behind make_grm(inverse = TRUE) (reference src/rm.cpp:39-42: solve() -> solver_chol(), src/solver.cpp:159-202: LAPACK dpotrf('L'),
 * dpotri('L') and the mirror) on the device: a right-looking blocked Cholesky, the factor's inverse (dtrtri) and the
 * product (dlauum), GEMM-shaped on the fp64 matrix cores. Matrices are n x n column-major fp64 device matrices of the interface above
 * (hb_eig_upload / hb_eig_download / hb_eig_release) or hb_grm_build's G_dev (lda = n). No floating-point atomics: two runs on the same matrix
 * agree bit for bit; no kernel waits for another workgroup. Refused before any device is asked for, HB_ERR_INVALID: a null pointer, n < 1,
 * lda < n, a non-finite lambda. Without a device: HB_ERR_NO_DEVICE. A work buffer that does not fit: HB_ERR_HIP with "out of memory" in the
 * text. solver_lu() (src/solver.cpp:204-249), the route the reference takes when dpotrf fails, stays with the caller (*info > 0).
 * ------------------------------------------------------------------------------------ */
/* dpotrf('L') in place: the lower triangle of A_dev + lambda*I becomes L; the strict upper triangle is neither read nor written.
 * *info = 0, or k > 0: the leading minor of order k is not positive definite (or its pivot is not finite); A_dev is then as the
 * factorisation left it. Returns HB_OK in both cases. */
int hb_chol_factor(double *A_dev, int64_t lda, int32_t n, int32_t device, double lambda, int32_t *info);
/* dtrtri('L','N') in place on hb_chol_factor's result */
int hb_chol_invert_factor(double *L_dev, int64_t lda, int32_t n, int32_t device);
/* solver_chol() (src/solver.cpp:159-202): A_dev <- (A_dev + lambda*I)^-1, both triangles, from A_dev's lower triangle. Works in a
 * buffer of its own: with *info > 0 (HB_OK) A_dev is untouched bit for bit, so the caller can take solver_lu()'s route. The result
 * equals its transpose bit for bit. Allocates bytes[2] of hb_chol_plan for the call: a second n x n matrix and an n x 256 block column. */
int hb_spd_inverse(double *A_dev, int64_t lda, int32_t n, int32_t device, double lambda, int32_t *info);
/* The plan of hb_cholplan.hpp for the tests, a pure function of n that needs no device: *nb the panel width, *ldw the work buffer's leading
 * dimension (even), bytes[3] what hb_chol_factor, hb_chol_invert_factor and hb_spd_inverse allocate, and per panel of the factorisation
 * (*nsteps of them; cap: the length of every array, ceil(n / 64) suffices) its first column k0, its width, the 64-row tiles of the panel
 * below its diagonal block and the 64 x 64 tiles of the trailing matrix's lower triangle. */
int hb_chol_plan(int32_t n, int32_t cap, int32_t *nb, int64_t *ldw, int64_t *bytes, int32_t *nsteps, int32_t *k0, int32_t *width, int32_t *row_tiles,
                 int64_t *tri_tiles);

/* ====================================================================================
 * Fine-grained engine API.  hb_bayes_run() is built on it; the parity tests and bench.py
 * drive the device pieces through it one at a time.  A context owns all device state of
 * one genotype shard; calls on one context must be serialised by the caller.
 * ==================================================================================== */
typedef struct hb_ctx_params {
    int32_t device;
    int32_t n, m;            /* individuals, local markers */
    int32_t panel;           /* 0 = auto */
    int32_t precise;
    int64_t m_offset;        /* global index of local marker 0 (RNG addressing) */
    uint64_t seed;
} hb_ctx_params;

int hb_ctx_create(const hb_ctx_params *p, hb_ctx **out);
void hb_ctx_destroy(hb_ctx *c);
int hb_ctx_panel(const hb_ctx *c);
int64_t hb_ctx_ld(const hb_ctx *c);     /* device leading dimension of X in bytes */

/* Genotypes -> device int8, column-major. ncols columns starting at col0. For both upload calls X is the address of the
 * first uploaded column (the source of device column col0), with ld >= n elements from one column to the next. */
int hb_ctx_upload_genotype_i8(hb_ctx *c, const int8_t *X, int64_t ld, int32_t col0, int32_t ncols);
/* doubles are checked for integrality and range, never rounded silently */
int hb_ctx_upload_genotype_f64(hb_ctx *c, const double *X, int64_t ld, int32_t col0, int32_t ncols);
/* PLINK .bed (SNP-major, 2 bits/genotype) decoded ON DEVICE with the code map of reference
 * src/read_bed.cpp:116-120 and its major-genotype imputation (:182-230); `rows` (n long,
 * indices into the .bed's nind individuals) selects/reorders individuals as ibrm() does
 * (R/bayes.r:165, :286-291); NULL = first n individuals. bed excludes no header: pass the
 * whole file image including the 3 magic bytes. */
int hb_ctx_upload_bed(hb_ctx *c, const uint8_t *bed, int64_t nbytes, int32_t nind,
                      const int32_t *rows, int32_t col0, int32_t ncols);
/* synthetic genotypes generated on device (SURVEY §8 d): p_j ~ U(0.05,0.5),
 * x ~ Binomial(2,p_j), every mono_every-th column forced monomorphic (0 = never) */
int hb_ctx_generate_genotype(hb_ctx *c, uint64_t seed, int32_t mono_every);
int hb_ctx_download_genotype(hb_ctx *c, int8_t *X, int64_t ld, int32_t col0, int32_t ncols);
/* Real-valued genotypes (imputed dosages) -> the fp64 resident layout: column-major doubles with the row padding of the int8 columns. All m
 * columns at once, any finite value as it is; a NaN or Inf is HB_ERR_INVALID, "NAs are not allowed in genotype.". The context then stays on the
 * event-ordered per-panel kernels (hb_ctx_set_pipeline(1, ...) keeps pipeline 0, hb_ctx_pipeline_note tells why), hb_ctx_get_layout reports
 * 64, hb_ctx_build_gram builds the diagonal Gram block of each panel in fp64 (hb_ctx_download_gram_real), hb_ctx_dot / hb_ctx_matvec /
 * hb_ctx_matmul / hb_ctx_marker_stats / the sweeps read the doubles. hb_ldm_build, hb_grm_build and hb_ctx_set_layout(2 or 8) refuse such a
 * context (HB_ERR_UNSUPPORTED); an integer upload (hb_ctx_upload_genotype_i8 / _f64 / _bed) puts it back on the int8 columns.
 * hb_ctx_download_genotype_real gives the values back bit for bit. */
int hb_ctx_upload_genotype_real(hb_ctx *c, const double *X, int64_t ld);
int hb_ctx_download_genotype_real(hb_ctx *c, double *X, int64_t ld);
/* (bits = 64: the int8 columns converted to the fp64 resident layout on the device — see hb_ctx_upload_genotype_real.)
 * Resident layout the sweep's kernels read: bits = 8 (int8 columns) or 2 (2 bits per genotype: 16 individuals per 32-bit word,
 * expanded in registers — hb_dotq2.hpp; codes must be 0..3). Packing happens on the device from the int8 columns. keep_int8 = 0
 * frees the int8 copy afterwards (every kernel of the run — mat-vec, residual update, X*alpha, the GEBV sample matrix, genotype
 * download — then reads the packed form; the Gram blocks must have been built for the widest geometry the run will use, a
 * rebuild unpacks panel by panel into a scratch buffer). bits = 8 on a context that dropped its int8 copy unpacks it again. */
int hb_ctx_set_layout(hb_ctx *c, int32_t bits, int32_t keep_int8);
int hb_ctx_get_layout(const hb_ctx *c, int32_t *bits, int32_t *int8_resident);
/* Which kernel computes the panel mat-vec on 2-bit resident genotypes (ABI 5; all three produce the same exact integers, hence the same
 * chain bit for bit): 2 = k_dotq2m, the seven digit planes of the residual as a skinny int8 GEMM on the matrix cores
 * (v_mfma_i32_16x16x64_i8) — THE DEFAULT since round 5 (12 us per 3584-column launch at n = 50k against 22: with the residual held as
 * seven int8 planes the product [columns x individuals] x [individuals x 7] is a dense integer contraction, and the v_dot4 form is bound
 * by vector-ALU issue, not by memory); 0 = k_dotq2, lane = column, v_dot4_i32_i8 (north_star's literal "coalesced loads with LDS-staged
 * wavefront reductions, no MFMA"; the default until round 4, kept selectable and measured beside the default by bench.py); 1 = k_dotq2r,
 * individuals across the lanes. Also HB_DOTQ2_KIND. The int8-column layout (the library's default layout) always runs k_dotq: v_dot4, no MFMA. */
int hb_ctx_set_matvec_kernel(hb_ctx *c, int32_t kind);

/* xpx_i = sum x^2, vx_i = var(x_i) (N-1), reference src/Bayes.cpp:310-317; integer-exact (the fp64 resident layout: two passes, arma::var's
 * form; a column of one repeated value has vx == 0 exactly) */
int hb_ctx_marker_stats(hb_ctx *c, double *xpx, double *vx, double *sumvx, int32_t *nvar0);
/* Pipeline geometry of the sweep: pipeline 0 = one kernel per step and panel, 1 = persistent
 * chain workgroup overlapped with the mat-vec stream; `lookahead` mat-vec groups of `dotgroup` panels each run
 * ahead of the chain. Results do not depend on it: the same chain — identical decisions and move lists, effects to 1e-9 (two
 * geometries add the band corrections to a right-hand side in different orders). A band wider than the stored one rebuilds the Gram blocks.
 * What hb_bayes_run picks for a context it creates (end of round 6): (1, 2, 7) for BayesB / BayesC, with (1, 2, 2) while many markers move; (1, 2, 2) /
 * (1, 2, 1) for BayesR; (1, 2, 2) for BayesRR / A / L at panel 512. A geometry the band limit cannot hold is narrowed (hb_ctx_get_pipeline tells): at most 20
 * panels of band, 27 with the forward workgroup beside the group chain — panel 512: (3, 7) and (2, 8). */
int hb_ctx_set_pipeline(hb_ctx *c, int32_t pipeline, int32_t lookahead, int32_t dotgroup);
/* per-panel Gram blocks G = X_p' X_p (int32, exact) plus the look-ahead band; also reports seconds spent */
int hb_ctx_build_gram(hb_ctx *c, double *seconds);
/* rows x cols window of panel p's Gram (row-major int32, P x P) for exactness tests */
int hb_ctx_download_gram(hb_ctx *c, int32_t panel_index, int32_t *G);
/* its twin on the fp64 resident layout: panel p's Gram block as row-major doubles, P x P — symmetric bit for bit, its diagonal the xpx of
 * hb_ctx_marker_stats bit for bit */
int hb_ctx_download_gram_real(hb_ctx *c, int32_t panel_index, double *G);
/* band block l of panel p (row-major int32, P x P): G[k][t] = x_{(p-l)P+k} . x_{pP+t}, l = 0..band; the look-ahead
 * pipeline folds the moves of panel p-l into panel p's right-hand sides with it */
int hb_ctx_download_gram_band(hb_ctx *c, int32_t panel_index, int32_t l, int32_t *G);
/* NULL when the persistent pipeline is available; otherwise the reason the context fell back to the event-ordered
 * per-panel kernels (kernels on two streams are not co-resident here: AMD_SERIALIZE_KERNEL, HIP_LAUNCH_BLOCKING, a
 * counter-collecting profiler ...). Probed once at hb_ctx_create(); hb_ctx_set_pipeline(1, ...) then keeps pipeline 0.
 * A context on the fp64 resident layout (hb_ctx_upload_genotype_real) also has a note: that layout runs on the per-panel kernels only. */
const char *hb_ctx_pipeline_note(const hb_ctx *c);
/* Geometry by regime. The band Gram blocks are stored once, for the widest band built so far; hb_ctx_set_pipeline() to any
 * geometry whose band fits reuses them (and the sweeps captured for each geometry are cached). With adaptive != 0,
 * hb_bayes_run / hb_run_step choose the geometry of each sweep of a point-mass model (BayesB/C) from the number of markers that
 * moved in the previous one: a narrow band while many move (every move costs one band row per block), the wide band with its
 * big mat-vec launches once few do. Same chain either way. hb_bayes_run does this by itself for a context it creates. */
int hb_ctx_set_adaptive(hb_ctx *c, int32_t adaptive);
/* current geometry: pipeline flag, look-ahead groups, panels per mat-vec launch, band width (blocks l = 1..band) */
int hb_ctx_get_pipeline(const hb_ctx *c, int32_t *pipeline, int32_t *lookahead, int32_t *dotgroup, int32_t *band);
/* move lists of the last sweep: ev_count[npanels]; ev_idx / ev_delta are [npanels][P] with ev_count[p] valid entries
 * (marker index inside the panel, change of its effect), in the order the chain applied them */
int hb_ctx_get_events(hb_ctx *c, int32_t *ev_count, int32_t *ev_idx, double *ev_delta);

/* residual yadj and u = Xg (n each) */
int hb_ctx_set_residual(hb_ctx *c, const double *yadj, const double *u);
int hb_ctx_get_residual(hb_ctx *c, double *yadj, double *u);
int hb_ctx_set_effects(hb_ctx *c, const double *g, const uint8_t *tracker, const double *vargL);
int hb_ctx_get_effects(hb_ctx *c, double *g, uint8_t *tracker, double *vargL);
/* d[j] = x_j . yadj for ncols columns from col0 — the panel mat-vec kernel on its own */
int hb_ctx_dot(hb_ctx *c, int32_t col0, int32_t ncols, double *d);

/* out (n) = X * alpha (m): the product behind e = y - ... - X*alpha, reference src/Bayes.cpp:971 */
int hb_ctx_matvec(hb_ctx *c, const double *alpha, double *out);

/* out (n x R, column-major, leading dimension ldo) = X * A, A (m x R, leading dimension ldA) on the host: the GEBV sample
 * matrix MCMCsamples$g = M %*% MCMCsamples$alpha of reference R/bayes.r:303-305 (then g$gebv = its row means, :308).
 * Eight records per pass, only over the columns with a non-zero effect in any of them. */
int hb_ctx_matmul(hb_ctx *c, const double *A, int64_t ldA, int32_t R, double *out, int64_t ldo);

/* The variance explained by windows of markers, item (8) of the reference README ("phenotypic/genetic variance explained (PVE) by single
 * or multiple SNPs"), which the reference leaves to the R session after the GEBV step of R/bayes.r:303-308. For every record r (column of
 * A, m x R, leading dimension ldA, on the host) and every window w (windindx: m ids in 1 .. nw):
 *     var_out[r * ldv + (w - 1)] = var over the n individuals of g_w = X_w alpha_w,r, N - 1 denominator (R's var),
 *     total_out[r]               = var(X alpha_r),
 * from the resident genotypes of any layout (int8, 2-bit, fp64), eight records per pass over the columns with a non-zero effect in any of
 * them (hb_pve.hip). Neither X alpha nor the n x nw matrix of window breeding values is ever stored. A window without a non-zero effect in a
 * record's batch is not visited and gets 0.0 exactly. Deterministic, and a (window, record) value depends on that window's effects of
 * that record alone: not on the other records, windows or ids. HB_ERR_INVALID: n < 2, a window id outside 1 .. nw, a non-finite effect, no
 * genotypes on the device; HB_ERR_UNSUPPORTED: a row-sharded context (shard_rows). */
int hb_ctx_window_var(hb_ctx *c, const double *A, int64_t ldA, int32_t R, const uint32_t *windindx, int32_t nw, double *var_out, int64_t ldv,
                      double *total_out);
/* The plan of one batch (hb_pveplan.hpp) for the tests; needs no device. A: m x nr effects, nr <= 8; s1: the m column sums over the n
 * individuals; ld: rows of a resident column. Every array holds m entries of its kind: idx[m] the list (marker columns, sorted by window and
 * marker), val[8 m] its effects, segs[3 m] (window 0-based, first entry, count) per window with an entry, shift[8 m] the segments' mean breeding
 * values, total_shift[8] that of the whole list, chunks[2 m] (first segment, count) per column of workgroups; counts[4] = entries, segments,
 * chunks, row blocks of 1024 rows. The launch is row blocks x chunks workgroups, and one more column for the total. */
int hb_pve_plan(const double *A, int64_t ldA, int32_t m, int32_t nr, const uint32_t *windindx, int32_t nw, const double *s1, int32_t n, int64_t ld,
                int32_t num_cus, int32_t *counts, int32_t *idx, double *val, int32_t *segs, double *shift, double *total_shift, int32_t *chunks);

/* The same item (8) for the summary-level model, where there are no genotypes: sbrm() (R/sbayes.r:231-234) returns the windows' WPPA and leaves
 * the variance they explain to the R session. The quantity is the quadratic form on the LD matrix of the handle, from the copy its kind reads —
 * HB_LDM_KIND_DENSE the dense device copy, every other kind the device CSC (nothing m x m is allocated for those) — (hb_ldquad.hip). For every
 * record r (column of A, rows x R with rows == m, leading dimension ldA, on the host, finite) and every window w (windindx: m ids in 1 .. nw,
 * a window's markers need not be contiguous):
 *     var_out[r * ldv + (w - 1)] = sum_{j in w} alpha_jr t_jr,  t_jr = sum_{i in w, (i, j) stored} V_ij alpha_ir,
 *     total_out[r]               = sum_j alpha_jr T_jr,         T_jr = sum_{i, (i, j) stored} V_ij alpha_ir,
 * eight records per pass over the columns with a non-zero effect in any of them. Every term is selected, (alpha != 0 ? V alpha : 0.0), so a
 * NaN or Inf entry (the sparse kinds keep NaN for monomorphic markers) reaches a result only where both effects are non-zero. Nothing is
 * clamped: a thresholded matrix is indefinite and a negative form is stored as computed. A window without a non-zero effect in a record's
 * batch is not visited and gets 0.0 exactly. Deterministic, no floating-point atomics; a (window, record) value depends on that window's
 * effects of that record alone: not on the other records, windows or ids. HB_ERR_INVALID: a null handle, rows != m, R < 1, a non-finite
 * effect, a window id outside 1 .. nw. */
int hb_ldm_window_var(hb_ldm *ldm, const double *A, int64_t ldA, int32_t rows, int32_t R, const uint32_t *windindx, int32_t nw, double *var_out,
                      int64_t ldv, double *total_out);
/* out[j] = V_jj for the m markers, from the copy the handle's kind reads (0.0 where a sparse matrix stores no diagonal entry) */
int hb_ldm_diagonal(hb_ldm *ldm, double *out);

/* helpers for the host blocks that share yadj (reference src/Bayes.cpp:479-516) */
int hb_ctx_residual_sums(hb_ctx *c, double *sum_r, double *sum_r2);
int hb_ctx_residual_shift(hb_ctx *c, double a);                       /* yadj += a        */
int hb_ctx_set_covariates(hb_ctx *c, const double *Cmat, int32_t nc); /* n x nc, col-major */
int hb_ctx_cov_dot(hb_ctx *c, int32_t i, double *out);                /* C_i . yadj        */
int hb_ctx_cov_axpy(hb_ctx *c, int32_t i, double a);                  /* yadj += a C_i     */
int hb_ctx_set_levels(hb_ctx *c, const int32_t *zid, int32_t nr, const int32_t *nlev);
int hb_ctx_level_sums(hb_ctx *c, int32_t term, double *sums);         /* Z_t' yadj         */
int hb_ctx_level_axpy(hb_ctx *c, int32_t term, const double *delta);  /* yadj += Z_t delta */

/* The covariate and random-effect blocks of one iteration (src/Bayes.cpp:484-516) as device kernels with no host
 * synchronisation: the caller draws the deviates first, in the reference's order (they do not depend on the data) —
 * z_beta[nc], then per term its level normals (z_levels, all terms concatenated) and chisq[term] = chisq_sample(q_t + dfr) —
 * and reads the state back whenever it needs it (hb_ctx_blocks_state synchronises). set_covariates / set_levels first. */
int hb_ctx_blocks_setup(hb_ctx *c, const double *cpc /* nc */, const double *zz /* levels */, const double *vrtmp0 /* nr */);
int hb_ctx_blocks_step(hb_ctx *c, double vare, const double *z_beta, const double *z_levels, const double *chisq, double dfr, double s2r);
int hb_ctx_blocks_state(hb_ctx *c, double *beta, double *estR, double *vrtmp, double *vr);

/* BSLMM's polygenic block of one iteration (src/Bayes.cpp:518-552) as device kernels with no host synchronisation, on the eigenvectors
 * Ki (n x n column-major, leading dimension ld >= n) and eigenvalues Kival (n, host) of the relationship matrix.
 * setup: on_device != 0 — Ki is a DEVICE pointer the context borrows (16-byte aligned, ld even; a torch tensor's data_ptr()); else a host
 * matrix that is uploaded (n * n * 8 bytes of device memory). Kival = Ki = NULL drops the block.
 * step: k_new = K ((eval / vare) o K'(yadj + k_old) + sqrt(max(eval, 0)) o z), eval = Kival vare / (Kival + vare / vb) (:531-535), z_j drawn on
 * the device (Philox purpose 5: sub = (5 << 56) | iter, blk = j); yadj += k_old - k_new, u -= k_old - k_new (:537-540);
 * vb = (sum_j (K' k_new)_j^2 / Kival_j + s2_df) / chis (:543-547) with chis = chisq_sample(dfvara + n) drawn by the caller and
 * s2_df = s2vara * dfvara. vb_in < 0 uses the vb the previous step left on the device (the first step needs vb_in = vara, :333).
 * state: synchronises; k (n) = the polygenic vector, *flag != 0 = the check of :533 failed in the last step (the sampler then fails with the
 * reference's text). Inside hb_run_step vb, q and the flag come back with the sweep's fetch. */
int hb_ctx_poly_setup(hb_ctx *c, const double *Kival, const double *Ki, int64_t ld, int32_t on_device);
int hb_ctx_poly_step(hb_ctx *c, double vare, double vb_in, uint64_t seed, int64_t iter, double chis, double s2_df);
int hb_ctx_poly_state(hb_ctx *c, double *k, double *vb, double *q, int32_t *flag);
/* Debug read-out for the kernel-level tests (tests/test_gpu_bslmm.py): what the last step left, n doubles each, any pointer may be NULL —
 * t = K'(yadj + k_old), w (the vector K multiplies), eval, Kg = K' k_new. Synchronises and changes nothing. */
int hb_ctx_poly_debug_get(hb_ctx *c, double *t, double *w, double *eval, double *Kg);

/* The single-step model's epsilon block of one iteration (src/Bayes.cpp:554-584) as device kernels with no host synchronisation (DESIGN.md
 * section 18). setup copies the descriptor's arrays, y_J (n) and index (ne, 1-based), validates them as hb_epsl_check does and builds the
 * schedule; epsilon and J start at 0. desc == NULL drops the block.
 * step: J (:555-564) with the caller's normal zJ; the Gibbs pass over the q rows (:565-576), row i drawing the normal of Philox purpose 6 at
 * blk = i; veps = (x'Gx + s2_df) / chis (:577-583) with chis = chisq_sample(dfvara + q) drawn by the caller. veps_in < 0 uses the veps the
 * previous step left on the device (the first step needs veps_in = vara, :332). yadj, its fp32 image and u stay coherent.
 * state: synchronises; x (q) = epsilon. Inside hb_run_step veps, q and J come back with the sweep's fetch. */
typedef struct hb_epsl_desc {
    const hb_epsl_gi *Gi;
    const uint32_t *index;
    const double *y_J;
} hb_epsl_desc;
int hb_ctx_epsl_setup(hb_ctx *c, const hb_epsl_desc *desc);
int hb_ctx_epsl_step(hb_ctx *c, double vare, double veps_in, uint64_t seed, int64_t iter, double zJ, double chis, double s2_df);
int hb_ctx_epsl_state(hb_ctx *c, double *x, double *veps, double *q, double *J);
/* Debug read-out and setter for the kernel-level tests (tests/test_gpu_epsl.py): what the last step left — b (q), the epsilon it started
 * from (q), the J draw's y_J . yadj —, counts[4] as hb_epsl_plan's; any pointer may be NULL. debug_set rebuilds the schedule under forced
 * modes (hb_epsl_plan's): the chain must not change by a bit. Both synchronise. */
int hb_ctx_epsl_debug_get(hb_ctx *c, double *b, double *x_old, double *rhs, int32_t *counts);
int hb_ctx_epsl_debug_set(hb_ctx *c, int32_t sched_mode, int32_t row_mode);

/* ssbrm()'s imputation on the device (R/ssbayes.r:295-307: Mn = solve(A^-1_nn, -A^-1_ng M), Jn beside it) without a factor: a batched
 * conjugate-gradient solve with the Jacobi preconditioner, hb_impute.hip, DESIGN.md section 19. Additive under ABI 6.
 * create (R/ssbayes.r:295-307, the two blocks of A^-1): A_nn, q x q, as canonical CSC with BOTH triangles stored, and A_ng, ng_rows x n_g, as
 * canonical CSR, both 0-based. Validated before any device call, each case with its own text (HB_ERR_INVALID): indptr from 0 and not
 * decreasing; indices sorted, unique and in range; finite values; ng_rows == q; a positive diagonal of A_nn; A_nn equal to its transpose in
 * pattern and in value bits. Then the matrices are copied to `device`; without one: HB_ERR_NO_DEVICE, as every compute entry point. */
typedef struct hb_impute hb_impute;
int hb_impute_create(int32_t q, const int64_t *nn_indptr, const int32_t *nn_indices, const double *nn_data, int32_t ng_rows, int32_t n_g,
                     const int64_t *ng_indptr, const int32_t *ng_indices, const double *ng_data, int32_t device, hb_impute **out);
typedef struct hb_impute_stats {
    int32_t width;          /* W: right-hand sides per block, a multiple of 64 (hb_imputeplan.hpp)                          */
    int32_t iterations;     /* until every column had stopped; the largest over the blocks                                  */
    int32_t blocks;         /* blocks of W columns solved one after the other                                               */
    int32_t parts;          /* partial sums per column: a function of q alone                                               */
    int32_t cached;         /* the plan expects the block of search directions to stay in the Infinity Cache                */
    int32_t looks;          /* host looks at the stop words                                                                 */
    double max_residual;    /* largest ||b - A_nn x|| / ||b|| over the columns, from one more product after the stop         */
    double seconds;         /* wall time of the call                                                                        */
    double product_seconds; /* HB_IMPUTE_PROFILE set: one launch of the product kernel alone, averaged over ten; else 0     */
    int64_t product_bytes;  /* bytes one launch of the product kernel moves at this width                                   */
} hb_impute_stats;
/* solve (R/ssbayes.r:295-307, a chunk of columns): M, n_g x ncols column-major with leading dimension ld, into Mn, q x ncols column-major
 * with leading dimension ld_out. A column stops at the first iteration with ||r|| <= tol ||b|| and is frozen there; a column with b = 0 is
 * exactly 0. tol outside (0, 1) or max_iter < 1: HB_ERR_INVALID (checked first). A column still live after max_iter iterations, or p'Ap <= 0:
 * HB_ERR_INVALID with the count in the text, and Mn is not a result. stats may be NULL. Two calls give the same bits, and a column's bits do
 * not depend on the columns solved beside it. */
int hb_impute_solve(hb_impute *h, const double *M, int64_t ld, int32_t ncols, double tol, int32_t max_iter, double *Mn, int64_t ld_out,
                    hb_impute_stats *stats);
/* destroy (R/ssbayes.r:295-307 needs the matrices no longer): frees the device copies; NULL is allowed */
void hb_impute_destroy(hb_impute *h);

/* One marker sweep (reference src/Bayes.cpp:586-816) plus the two reductions behind
 * :819 and :823.  Hyper-parameters come from the host, per-SNP draws happen on device. */
typedef struct hb_sweep_in {
    int32_t model_index;     /* 1 RR, 2 A, 3 B/Bpi, 4 C/Cpi, 5 L, 6 R   (:97)              */
    int32_t n_fold;
    int64_t iter;            /* addresses the marker RNG stream                             */
    double vare;
    double varg;             /* shared marker variance (RR, C, R)                           */
    double s2varg_df;        /* s2varg_ * dfvara_ (A, B)                                    */
    double dfvara;           /* (A, B)                                                      */
    double logpi[HB_MAX_FOLD];
    double fold[HB_MAX_FOLD];
    double vara_fold[HB_MAX_FOLD];
    double lambda, lambda2;  /* (L)                                                         */
    int32_t count_pip;       /* iter >= nburn: accumulate nzrate / window flags             */
    int32_t store;           /* thinned record: accumulate alpha moments                    */
} hb_sweep_in;

typedef struct hb_sweep_out {
    double sum_g2;            /* g.g (RR) | sum g^2 of included (C) | sum g^2/fold (R)      */
    double class_count[HB_MAX_FOLD]; /* markers per class among polymorphic ones, class 0
                                        EXCLUDES monomorphic markers                         */
    double sum_vargL;         /* (L) sum over markers incl. untouched monomorphic ones      */
    double sum_r, sum_r2;     /* over yadj after the sweep                                   */
    double var_u;             /* var(u), N-1                                                 */
    double n_events;          /* markers whose effect changed                                */
    double n_cache_miss;      /* ... of which the Gram row was not in the chain's LDS row cache */
    double n_redo;            /* speculative chain rounds that were rolled back and repeated    */
} hb_sweep_out;

int hb_ctx_sweep(hb_ctx *c, const hb_sweep_in *in, hb_sweep_out *out);
/* The same sweep in pieces, for a caller that exchanges residual deltas between them (hb_bayes_args.sync_blocks does exactly
 * this): block b of nblocks enqueues the panels of its share of the mat-vec groups as a self-contained pipeline — block 0 also
 * prepares the sweep, the last block closes it — and returns without waiting; hb_ctx_sweep_end() then fetches the sweep's sums.
 * The residual may be modified on the context's stream between two blocks (hb_ctx_set_residual / an all-reduce on it).
 * nblocks == 1 is hb_ctx_sweep() split into begin and end. */
int hb_ctx_sweep_range(hb_ctx *c, const hb_sweep_in *in, int32_t block, int32_t nblocks);
int hb_ctx_sweep_end(hb_ctx *c, hb_sweep_out *out);
/* nzrate counters (m, as doubles), alpha sum / sum of squares over stored records */
int hb_ctx_get_counters(hb_ctx *c, double *nzrate, double *alpha_sum, double *alpha_sq);
int hb_ctx_set_windows(hb_ctx *c, const uint32_t *windindx, int32_t nw);
int hb_ctx_get_windows(hb_ctx *c, double *wppa);

/* device timing of the last hb_ctx_sweep: milliseconds by phase, averaged per launch */
typedef struct hb_sweep_timing {
    double total_ms;
    double dot_ms;       /* summed over panel launches */
    int32_t dot_launches;
    double chain_ms;
    double update_ms;
    double other_ms;
} hb_sweep_timing;
int hb_ctx_last_timing(hb_ctx *c, hb_sweep_timing *t);
/* measurement helper: the panel mat-vec launches of one sweep, issued back to back exactly as the sweep issues them
 * (same columns per launch), timed with HIP events on the context's stream; average milliseconds per launch */
int hb_ctx_time_matvec(hb_ctx *c, int32_t reps, double *avg_ms, int32_t *launches_per_sweep, int32_t *cols_per_launch);
/* measurement helper ("fraction of a measured streaming-read kernel on the same buffer"): the resident genotype buffer
 * (int8 columns, or the 2-bit words when that layout is set) read once front to back by a plain 16-bytes-per-lane kernel, nothing
 * computed, nothing written; average milliseconds per pass over `reps` passes (one untimed pass first) and the bytes of one pass */
int hb_ctx_time_stream_read(hb_ctx *c, int32_t reps, double *avg_ms, int64_t *bytes);
/* on: bit 0 HIP-event timing of the per-panel kernels (hb_ctx_last_timing), bit 1 cycle stamps inside the chain kernel,
 * bit 2 chain-alone diagnostic, bit 3 in-situ stamps of the mat-vec launches (hb_ctx_matvec_stamps) */
int hb_ctx_set_profiling(hb_ctx *c, int32_t on);
/* In-situ duration of the dominant kernel. With hb_ctx_set_profiling(c, 8) every block of every mat-vec launch of a sweep
 * records the device's constant 100 MHz clock at its start and at its end — the launches of the REAL sweep, with the chain
 * workgroup and the update rows running beside them, not an isolated replay. A launch's duration is max(end) - min(start)
 * over its blocks (what a kernel trace reports); the statistics are over the launches of the last sweep. span_ms = first
 * launch's start to last launch's end, so launches * avg_ms <= span_ms <= the sweep's wall time. */
typedef struct hb_launch_stats {
    int32_t launches;        /* full-width mat-vec launches of the last sweep (the statistics are over these) */
    int32_t launches_all;    /* ... all of them (the last launch of a sweep may cover fewer columns) */
    int32_t blocks;          /* blocks of the last launch looked at (update rows + finalize + tiles) */
    int32_t cols_per_launch;
    double avg_ms, min_ms, max_ms, sum_ms, span_ms;
} hb_launch_stats;
int hb_ctx_matvec_stamps(hb_ctx *c, hb_launch_stats *out);
/* Debug hook for the replay of an aborted sweep (ABI 5): the next `times` sweeps the persistent pipeline runs on the context are
 * aborted in mid-flight — the abort flag a timed-out waiter raises is set once the chain has published `panel` panels — so
 * hb_ctx_sweep_end() returns HB_ERR_ABORTED for them; hb_run_step() restores the saved state and replays (twice on the pipeline,
 * then on the per-panel kernels, which the hook does not touch). times <= 0 disarms it. */
int hb_ctx_debug_inject_abort(hb_ctx *c, int32_t panel, int32_t times);
/* Debug read-out for the kernel-level tests (tests/test_gpu_boundary.py): what k_pre left for the chain in the last sweep of the context —
 * the thresholds on rhs^2, 1/v and sd*z — as kpad rows of m_pad doubles each (m_pad = the markers rounded up to whole panels; kpad = 1,
 * or BayesR's n_fold - 1 rounded up to 3 or 7; rows and columns beyond the model's are (+inf, 0, 0)). Synchronises the context's stream and
 * changes nothing; any of the pointers may be NULL. Fails before the first sweep. */
int hb_ctx_debug_get_pre(hb_ctx *c, int32_t *kpad, double *thr, double *invv, double *sdz);
/* Debug read-out for the kernel-level tests (tests/test_gpu_update.py): the residual version that the last executed update rows wrote, with
 * its mirrors, as they lie on the device (ld = hb_ctx_ld() rows each, rows [n, ld) included). *slot: the version slot read (0 before the
 * first sweep: the residual between sweeps, which every other writer of the residual keeps in that slot); *bound_index: h of the group
 * (pipeline) or panel (per-panel kernels) whose moves those rows applied, so that mb[1 + h] is the bound their exponent came from (-1 before
 * the first sweep); r: the slot's ld doubles; r32: its ld floats; *ndigits: the number of digit planes copied — 7 under precise = 2, else 0
 * with rq and vexp left untouched; rq: ndigits x ld int8 digits, plane k at rq + k * ld, value = sum_k rq[k][i] 256^k = rint(r[i] 2^vexp);
 * *vexp: the slot's exponent; mb: the npanels + 2 bounds on max |yadj| (mb[0]: at the start of the last range of panels enqueued, mb[1 + h]:
 * after group or panel h). Synchronises the context's stream and changes nothing; any of the pointers may be NULL. */
int hb_ctx_debug_get_mirrors(hb_ctx *c, int32_t *slot, int32_t *bound_index, double *r, float *r32, int32_t *ndigits, int8_t *rq,
                             int32_t *vexp, double *mb);
/* Debug read-out for the kernel-level tests (tests/test_gpu_opening.py): the certificate of the group chain as hb_ctx_build_gram() left it —
 * G[k][j] = ga[k] gB[j] + c[k][j] with |c[k][j]| <= gcmax[k] over the stored band, ga = rint(s / 256), gB = rint(256 s / n), s the column sum.
 * *ok: 1 when the arrays stand for the band the next sweep would run on; 0 — a success, with ga, gB and gcmax left untouched — where there is
 * no certificate: HB_CERT=0, a row-sharded context, the fp64 resident layout, before a Gram build, and after an upload or a wider geometry
 * until the band is built again. *Lg: the band the arrays were built over (blocks l = 0..Lg per panel). ga, gB, gcmax: m_pad int32 each
 * (m_pad = the markers rounded up to whole panels). Synchronises the context's stream and changes nothing; any of the pointers may be NULL. */
int hb_ctx_debug_get_cert(hb_ctx *c, int32_t *ok, int32_t *Lg, int32_t *ga, int32_t *gB, int32_t *gcmax);
/* Debug read-out for the kernel-level tests (tests/test_gpu_opening.py): what the chain of the context's last pipelined sweep was given for its
 * opening. *nslot: the rows of the row cache the lists were laid out for; *kappa, *candf: the prediction's and the candidates' factors;
 * *has_opn: 1 when the 16-byte records were written (a certificate existed), else 0 with opn left untouched. thr0f: m_pad floats, the entry
 * threshold rounded down to float (NaN: monomorphic marker, -inf: marker in the model); opn: m_pad x 4 int32, {candidate threshold (a double,
 * low word first), the filter word, gB}; slot_of: m_pad int32, a marker's place in the row cache in units of 64 ints (-1: none, -2: monomorphic);
 * hotpack: npanels x 256 int32, per panel [0] rows that fit, [1] rows listed, [2] whole rows among those that fit, [3] the shift in pieces,
 * [4 ...] the listed markers (words beyond [4 + [1]) are undefined). Synchronises the context's stream and changes nothing; any of the
 * pointers may be NULL. Fails before the first pipelined sweep. */
int hb_ctx_debug_get_opening(hb_ctx *c, int32_t *nslot, double *kappa, double *candf, int32_t *has_opn, float *thr0f, int32_t *opn,
                             int32_t *slot_of, int32_t *hotpack);
/* Debug read-out for the ownership tests (tests/test_gpu_ownership.py): what the library holds in this process right now — *buffers: the device
 * and pinned host buffers allocated and not yet freed, over every context, run and handle and every buffer handed to the caller (hb_grm_build's
 * G_dev, hb_eig_upload's A_dev, ...); *bytes: their sizes added up. (0, 0) when the library is loaded, and back at its earlier value after every
 * destroy, free and release and after every call that fails. Needs no device and touches none; either pointer may be NULL. */
int hb_debug_live_buffers(int64_t *buffers, int64_t *bytes);

#ifdef __cplusplus
}
#endif
#endif
