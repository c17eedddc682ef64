// hb_kernels.hip — gfx950 kernels of the block-Gibbs marker sweep.
//
// One sweep (reference src/Bayes.cpp:586-816) is executed panel by panel; a panel is P
// consecutive markers.  For each panel:
//   k_dot      d = X_p' yadj                  bandwidth-bound int8 mat-vec (the dominant kernel)
//   k_chain    the serial conditional updates of the panel's markers, made exact by the panel
//              Gram matrix G = X_p' X_p:  after marker k moves by D_k, rhs_j -= G[k][j] D_k
//              for every later marker j of the panel  (== what the reference gets by updating
//              yadj with daxpy before the next ddot)
//   k_update   yadj -= X_p[:, changed] D,  u += X_p[:, changed] D
// Per-marker quantities that do not depend on the running rhs (the uniform and normal deviates,
// 1/v, sd*z, and the inclusion test rewritten as thresholds on rhs^2) are produced once per
// sweep by k_pre, so the serial part is a handful of fp64 operations per marker.
//
// ONE translation unit, by role in included files (round 5; the kernels share device globals — the wait bound, the abort log —
// and the view structs, which separate objects could only share through relocatable device code):
//   hand-offs        hb_handoff.hpp        flag block, sc1 loads / write-through stores, bounded waits
//                    hb_wave.hpp           wave and block sums, HB_INF (every unit with kernels includes it)
//   mat-vec          hb_matvec.hpp         k_dot, k_dotq (int8 columns)        hb_dotq2.hpp   k_dotq2 / k_dotq2r / k_dotq2m (2-bit)
//                    hb_update.hpp         the residual update rows that ride in the launches, and their dense form
//   per marker       hb_pre.hpp            pre_marker (thresholds, deviates), BayesL's draw, k_windows: shared with hb_sbayes_sparse.hip
//   chains           hb_chain_panel.hpp    k_chain (one kernel per panel)
//                    hb_chain_persist.hpp  k_chain_persist, k_hotlist          hb_chain_group.hpp  k_chain_group, k_fwd
//                    hb_chain_dense.hpp    k_chain_dense, k_fold_dense         hb_warm.hpp         k_gate, k_warm
//   host blocks      hb_blocks.hpp         intercept / covariates / random effects, delta pack / unpack
//                    hb_reduce.hpp         var(u), yadj.yadj, BayesL's variances
//   ingest / egress  hb_stats.hpp          xpx, vx                              hb_ingest.hpp  f64 check, .bed decode, X alpha, GEBV, generator
//   summary level    hb_sbayes.hpp         SBayesD on a dense LD matrix
//   host plans       hb_plan.hpp           which chain, k_fwd and warmers a sweep runs (plan_sweep: no HIP, tested on the CPU)
//                    hb_matvecplan.hpp     which kernel, tiling and LDS a mat-vec launch gets (plan_matvec: the same), the shapes' lists and LDS formulas
//   this file        sweep start (k_sweep_init, k_quant0, k_pre), the launch tables, the launchers, graph capture, probes, thin wrappers for hb_ctx.hip
#include "hb_internal.hpp"
#include "hb_plan.hpp"
#include "hb_rng.hpp"
#include <type_traits>
#include <algorithm>
#include <cstdlib>
#include <map>
#include <mutex>

#include "hb_handoff.hpp"
#include "hb_pre.hpp"
#include "hb_stats.hpp"
#include "hb_update.hpp"
#include "hb_matvec.hpp"
#include "hb_dotq2.hpp"

// Sweep start of the fixed-point path: max |yadj| -> mb[0] and the exponent of slot 0, then slot 0's digit planes.
// One workgroup (n is a few hundred KB).
__global__ __launch_bounds__(256) void k_sweep_init(double *__restrict__ acc, unsigned *__restrict__ flags, int32_t *__restrict__ ev_count,
                                                    int np, unsigned long long *__restrict__ dsum, int m_pad, int p_lo,
                                                    unsigned long long *__restrict__ fcorr, unsigned long long *__restrict__ dd,
                                                    unsigned long long *__restrict__ mbs, int mb_lo, int mb_hi,
                                                    unsigned long long *__restrict__ fc2, int32_t *__restrict__ ev_idx,
                                                    unsigned long long *__restrict__ ev_delta, int P)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    if (acc && i < HB_ACC_N) acc[i] = 0.0; // (null: a later range of the same sweep keeps the sums)
    // (a later range of the same sweep keeps an abort raised by an earlier one, and with it who gave up waiting for what — words 8..14
    // and the abort log's record count — which is what HB_DEBUG_ABORT prints)
    if (i < HB_NFLAGS && (acc || (i != HB_FLAG_ABORT && !(i >= 8 && i <= 14) && i != HB_FLAG_LOGN))) flags[i] = 0u;
    // move counts and list entries of the panels of this range on: "not written yet" (the update rows poll them directly; an earlier
    // range's move lists stay readable)
    for (int k = p_lo + i; k < np; k += stride) ev_count[(size_t)k * HB_EVS] = -1;
    for (size_t k = (size_t)p_lo * P + i; k < (size_t)np * P; k += stride) {
        ev_idx[k] = -1;
        ev_delta[k] = ~0ull;
    }
    for (int k = i; k < m_pad; k += stride) dsum[k] = ~0ull;
    if (fcorr)
        for (int k = i; k < m_pad; k += stride) fcorr[k] = ~0ull;
    if (dd)
        for (int k = i; k < m_pad; k += stride) dd[k] = ~0ull;
    if (fc2)
        for (int k = i; k < m_pad; k += stride) fc2[k] = ~0ull;
    if (mbs) // (the dense update rows poll the group's bound on max |yadj| together with its changes: "not written yet")
        for (int k = mb_lo + i; k < mb_hi; k += stride) mbs[(size_t)k * HB_MBS] = ~0ull;
}

// sweep start of the fixed-point path, in two steps that use the whole device (round 5: one workgroup of 1024 took 33 us over n = 50 000 —
// 49 dependent loads per thread, twice — and k_pre + k_hotlist beside it are done after 30): max |yadj| (exact in any order: the doubles
// are non-negative, so their bit patterns order like the numbers and one integer atomicMax per wave collects them; *out zeroed before),
// then the digits of every row on that exponent.
__global__ __launch_bounds__(256) void k_absmax(const double *__restrict__ r, int64_t ld, unsigned long long *__restrict__ out)
{
    double mx = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ld; i += (int64_t)gridDim.x * blockDim.x) mx = fmax(mx, fabs(r[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(out, (unsigned long long)__double_as_longlong(mx));
}

__global__ __launch_bounds__(256) void k_quant0(const double *__restrict__ r, int64_t ld, int8_t *__restrict__ rq, double *__restrict__ mb,
                                                int *__restrict__ vexp, const double *__restrict__ maxp)
{
    // (maxp: the word k_absmax left in mb[0], or — row-sharded mode — max |yadj| over ALL shards, so that every shard's digits share one exponent)
    const double m2 = *maxp;
    const int E = hb_fix_exp(m2);
    for (int64_t row0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; row0 < ld; row0 += (int64_t)gridDim.x * blockDim.x * 4)
        hb_store_digits(rq, ld, row0, E, r[row0], r[row0 + 1], r[row0 + 2], r[row0 + 3]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (maxp != mb) mb[0] = m2;
        vexp[0] = E;
    }
}

__global__ void k_sum_partials(const double *__restrict__ partial, int pstride, int nsplit, int ncols,
                               double *__restrict__ out)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ncols) return;
    double s = 0;
    for (int sp = 0; sp < nsplit; sp++) s += partial[(int64_t)sp * pstride + j];
    out[j] = s;
}

// k_pre: pre_marker under the sweep's one residual variance, for the markers [m_offset, m_offset + m) of the whole marker set
struct pre_view {
    int m, m_pad;
    int64_t m_offset;
    uint64_t seed;
    const double *xpx, *vx, *g, *vargL;
    double *thr, *invv, *sdz;
    int kpad; // thresholds written per marker (1, 3 or 7)
};

__global__ __launch_bounds__(256) void k_pre(const hb_sweep_in *__restrict__ pin, pre_view v)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= v.m_pad) return;
    pre_marker<false>(pin, v, j, pin->vare, v.m_offset + j);
}

// the sums of a sweep on the per-panel kernels start from zero: stores from a kernel, as k_sweep_init's on the pipeline
__global__ void k_zero_acc(double *__restrict__ acc)
{
    if (threadIdx.x < HB_ACC_N) acc[threadIdx.x] = 0.0;
}

#include "hb_chain_panel.hpp"
#include "hb_chain_persist.hpp"
#include "hb_chain_group.hpp"
#include "hb_chain_dense.hpp"
#include "hb_warm.hpp"
// ---------------------------------------------------------------------------------------------
// k_update: yadj -= sum_e x_e D_e, u += the same, r32 = (float)yadj, for the panel's changed markers.
// thread = 4 consecutive rows; the event list is staged in LDS once, then the column loads of 8
// events are in flight together.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_update_dense(int64_t ld, upd_view q)
{
    __shared__ __attribute__((aligned(16))) char smem[HBU_LDS];
    update_rows_dense(ld, q, blockIdx.x, gridDim.x, smem);
}

__global__ __launch_bounds__(256) void k_update(int64_t ld, upd_view q)
{
    __shared__ int s_ix[512];
    __shared__ double s_dl[512];
    update_rows(ld, q, blockIdx.x, s_ix, s_dl);
}

#include "hb_reduce.hpp"
#include "hb_blocks.hpp"
#include "hb_ingest.hpp"
// =============================================================================================
// host side: launchers
// =============================================================================================
// LDS budget of k_chain: as many Gram rows as fit beside the event lists
// (elem: bytes per Gram entry — 4, or 8 on the fp64 resident layout, whose rows are doubles)
static int chain_nslot(int P, int elem = 4) { return (int)((158 * 1024 - ((size_t)P * 16 + 128 + 128 + 64)) / ((size_t)P * elem)); }
#define HB_PERSIST_RING(P) ((size_t)4 * ((((size_t)12 * (P) + 1023) >> 10 << 10) + 1024)) /* HB_RD slots of the opening ring */
// move lists (12 B per marker) + reduction / counter words + one round's candidate staging (sized by the model's K1 non-null classes)
// + the 64 x 64 block of mutual Gram entries + the correction ring + the opening ring; the rest is the double-buffered row cache
#define HB_PERSIST_FIXED(P, LB, K1) ((size_t)(P) * 12 + 128 + 512 + 64 * (8 * (3 + 3 * (K1)) + 12) + 64 * 64 * 4 + (size_t)((LB) + 1) * (P) * 8 + HB_PERSIST_RING(P) + (size_t)2 * (P) * 8 /* k_fwd's sums, two panels */ + (72 + 64) * 16 /* a round's moves as the apply reads them */)
static int persist_nslot(int P, int Lb, int K1) { return std::min(P, std::min(250, (int)((160 * 1024 - HB_PERSIST_FIXED(P, Lb, K1)) / ((size_t)P * 4)))); }
// the whole 160 KiB: nothing that needs LDS (mat-vec, update) can then be co-scheduled on the chain's CU
static size_t persist_smem(int) { return (size_t)160 * 1024; }
static size_t chain_smem(int P, int elem = 4) { return (size_t)chain_nslot(P, elem) * P * elem + (size_t)P * 16 + 128 + 128 + 64; }
// the fixed-point mat-vec: precise = 2 on the integer layouts (the fp64 resident layout multiplies in fp64 whatever precise says)
static inline bool fixed_point(const hb_ctx *c) { return c->precise == 2 && c->layout != 64; }

// The launch tables: a sweep plan's template arguments (plan_sweep, hb_plan.hpp) -> the instantiation, one table per kernel family, expanded
// from the plan's own lists. The three chain tables are also the list of the kernels that ask for the whole 160 KiB of LDS (hbk_init_attrs).
template <int N, class... Params>
struct kernel_entry {
    int arg[N];             // template arguments
    void (*fn)(Params...);  // the kernel
};
#define HB_GROUP_ENTRY(K1, DM, FW, CH, CERT) {{K1, DM, FW, CH, CERT}, k_chain_group<K1, DM, FW, CH, (CERT) != 0>},
#define HB_PERSIST_ENTRY(K1, NPL) {{K1, NPL}, k_chain_persist<K1, NPL>},
#define HB_DENSE_ENTRY(LASSO) {{LASSO}, k_chain_dense<(LASSO) != 0>},
#define HB_FWD_ENTRY(D, G, CH) {{D, G, CH}, k_fwd<D, G, CH>},
static const kernel_entry<5, const hb_sweep_in *, chain_view, persist_view> group_chains[] = {HB_GROUP_KERNELS(HB_GROUP_ENTRY)};
static const kernel_entry<2, const hb_sweep_in *, chain_view, persist_view, int> persist_chains[] = {HB_PERSIST_KERNELS(HB_PERSIST_ENTRY)};
static const kernel_entry<1, const hb_sweep_in *, chain_view, persist_view, double *, const double *> dense_chains[] = {HB_DENSE_KERNELS(HB_DENSE_ENTRY)};
static const kernel_entry<3, chain_view, persist_view> fwd_kernels[] = {HB_FWD_KERNELS(HB_FWD_ENTRY)};

// null, and the error recorded: the caller names a kernel that was never built — a programming error, never a reason to run another instantiation
template <class E, size_t M>
static const E *find_kernel(const E (&tab)[M], const int *arg, const char *what)
{
    for (const E &e : tab)
        if (std::equal(std::begin(e.arg), std::end(e.arg), arg)) return &e;
    hb_fail(HB_ERR_INVALID, std::string(what) + ": template arguments that are in no launch table");
    return nullptr;
}

int hbk_init_attrs()
{
    auto lds160 = [](const void *k) { return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); };
    for (auto &e : persist_chains) HB_HIP(lds160(reinterpret_cast<const void *>(e.fn)));
    for (auto &e : group_chains) HB_HIP(lds160(reinterpret_cast<const void *>(e.fn)));
    for (auto &e : dense_chains) HB_HIP(lds160(reinterpret_cast<const void *>(e.fn)));
    HB_HIP(lds160(reinterpret_cast<const void *>(&k_chain<1>)));
    HB_HIP(lds160(reinterpret_cast<const void *>(&k_chain<3>)));
    HB_HIP(lds160(reinterpret_cast<const void *>(&k_chain<7>)));
    HB_HIP(lds160(reinterpret_cast<const void *>(&k_chain<1, double>)));
    HB_HIP(lds160(reinterpret_cast<const void *>(&k_chain<3, double>)));
    HB_HIP(lds160(reinterpret_cast<const void *>(&k_chain<7, double>)));
    return HB_OK;
}

template <int K1>
static hipError_t launch_chain(hb_ctx *c, const chain_view &cv, int p, hipStream_t st)
{
    if (c->layout == 64) // (cv.gram points at the fp64 Gram blocks)
        hipLaunchKernelGGL((k_chain<K1, double>), dim3(1), dim3(c->P), chain_smem(c->P, 8), st, c->d_in, cv, p, chain_nslot(c->P, 8));
    else
        hipLaunchKernelGGL(k_chain<K1>, dim3(1), dim3(c->P), chain_smem(c->P), st, c->d_in, cv, p, chain_nslot(c->P));
    return hipGetLastError();
}

// residual version v (moves of panels <= v applied; v = -1: start of the sweep) lives in slot (v+1) mod NB
static inline int ver_slot(const hb_ctx *c, int v) { return (v + 1) % c->NB; }

// One launch of the panel mat-vec as its caller describes it: the columns, and what the defaults leave out
struct dot_launch {
    int col0, ncols;                  // the launch's columns (whole panels)
    int slot = 0;                     // the residual slot it reads
    hipStream_t st = nullptr;         // (null: the context's stream)
    int gidx = 0;                     // its index in the sweep: exponent word, block stamps, time-out diagnostics
    const upd_view *upd = nullptr;    // the update rows that ride in it
    int fin_col0 = 0, fin_ncols = 0;  // the columns of launch gidx - 1, whose sums it finalizes (fixed point) or reduces (k_dot)
};

// the built shapes of the 2-bit mat-vec (hb_dotq2.hpp), expanded from the plan's own lists (hb_matvecplan.hpp): {HB_MV_DOTQ2M, CT, G, SC}, {HB_MV_DOTQ2, CPL, RS, 0}
#define HB_Q2M_ENTRY(CT, G, SC) {{HB_MV_DOTQ2M, CT, G, SC}, k_dotq2m<CT, G, (SC) != 0>},
#define HB_Q2_ENTRY(CPL, RS) {{HB_MV_DOTQ2, CPL, RS, 0}, k_dotq2<CPL, RS>},
static const kernel_entry<4, dq_view, upd_view> dotq2_kernels[] = {HB_DOTQ2M_KERNELS(HB_Q2M_ENTRY) HB_DOTQ2_KERNELS(HB_Q2_ENTRY)};
// the update rows that ride in a launch stage their move lists at the head of the block's dynamic LDS (k_dotq2r, which asks for none, has a buffer of its own)
#define HB_Q2M_HOLDS(CT, G, SC) static_assert(q2m_lds(CT, G) >= HBU_ROWS_LDS, "k_dotq2m: a shape's LDS does not hold the update rows' move lists");
#define HB_Q2_HOLDS(CPL, RS) static_assert(q2_lds(CPL, RS) >= HBU_ROWS_LDS, "k_dotq2: a shape's LDS does not hold the update rows' move lists");
HB_DOTQ2M_KERNELS(HB_Q2M_HOLDS) HB_DOTQ2_KERNELS(HB_Q2_HOLDS)
static_assert(HBQ_LDS >= HBU_ROWS_LDS, "k_dotq: its LDS does not hold the update rows' move lists");

// One launch of the fixed-point mat-vec (k_dotq, k_dotq2, k_dotq2m, k_dotq2r). WHAT it is — kernel, template arguments, stages per tile, tiles, blocks,
// LDS — is plan_matvec's answer (hb_matvecplan.hpp, tested on the CPU); here the launch is described, the view filled, the block count registered.
static int launch_dotq(hb_ctx *c, const dot_launch &l, hipStream_t st)
{
    const upd_view uq = l.upd ? *l.upd : upd_view{};
    const int gidx = l.gidx;
    // the residual slot's digits and exponent, the plane sums, the update and finalize rows that ride in the launch, the finalize window
    dq_view v{};
    v.ld = c->ld;
    v.rq = c->rq + (size_t)l.slot * HB_ND * c->ld;
    v.vexp_in = c->vexp + l.slot;
    v.gexp_out = c->gexp + gidx;
    v.accq = c->accq + l.col0;
    v.accstride = c->m_pad;
    v.nupd = (uq.p1 > uq.p0) ? (int)(c->ld / (uq.dense ? 64 : 256)) : 0;
    v.nfin = l.fin_ncols > 0 ? (l.fin_ncols + 63) / 64 : 0;
    v.fin_acc = c->accq + l.fin_col0;
    v.fin_out = c->dsum + l.fin_col0;
    v.fin_exp = c->gexp + gidx - 1;
    v.fin_ncols = l.fin_ncols;
    if (c->layout == 2) {
        v.X2 = reinterpret_cast<const uint8_t *>(c->X2) + (int64_t)l.col0 * c->ld2;
        v.ld2 = c->ld2;
    } else v.X = c->X + (int64_t)l.col0 * c->ld;
    const hb_matvec_plan p = plan_matvec(hb_matvec_shape{c->layout, c->ld, c->ld2, l.ncols, v.nupd, v.nfin, uq.dense != 0, c->num_cus}, c->mv);
    v.nstages = p.nstages;
    v.NS = p.NS;
    v.ncg = p.ncg;
    // the launch's blocks, for the block stamps and the time-out diagnostics
    v.ldiag = (c->ldiag && gidx >= 0 && gidx <= c->npanels) ? c->ldiag + 4 * (size_t)gidx : nullptr;
    if (v.ldiag) c->ldiag_nblk[gidx] = p.blocks;
    if (c->lstamp && gidx >= 0 && gidx <= c->npanels && p.blocks <= HB_LSTAMP_BLOCKS) {
        v.stamp = c->lstamp + (size_t)gidx * HB_LSTAMP_BLOCKS * 2;
        c->lstamp_nblk[gidx] = p.blocks;
        c->lstamp_cols[gidx] = l.ncols;
    }
    void (*fn)(dq_view, upd_view) = p.family == HB_MV_DOTQ ? k_dotq : p.family == HB_MV_DOTQ2R ? k_dotq2r : nullptr;
    if (!fn) { // (the families with a table)
        const int shape[4] = {p.family, p.arg[0], p.arg[1], p.arg[2]};
        const auto *k = find_kernel(dotq2_kernels, shape, p.family == HB_MV_DOTQ2M ? "k_dotq2m" : "k_dotq2");
        if (!k) return HB_ERR_INVALID;
        fn = k->fn;
    }
    hipLaunchKernelGGL(fn, dim3(p.blocks), dim3(64), p.lds, st, v, uq);
    return HB_OK;
}

static int launch_dot(hb_ctx *c, const dot_launch &l)
{
    hipStream_t st = l.st ? l.st : c->stream;
    if (c->layout == 64) return hbk_real_dot(c, l.col0, l.ncols, c->r + (size_t)l.slot * c->ld, st); // (per-panel route only: nothing rides in the launch)
    if (c->precise == 2) return launch_dotq(c, l, st);
    upd_view uq{};
    if (l.upd) uq = *l.upd;
    const dim3 grid(l.ncols / 8, c->nsplit + (uq.p1 > uq.p0 ? 1 : 0) + (l.fin_ncols > 0 ? 1 : 0)), block(256);
    const int8_t *Xp = c->X + (int64_t)l.col0 * c->ld;
    double *part = c->partial + l.col0;
    const float *r32 = c->r32 + (size_t)l.slot * c->ld;
    const double *r64 = c->r + (size_t)l.slot * c->ld;
    const bool sgn = c->xmin < 0;
    dot_sync sy{c->partial + l.fin_col0, c->dsum + l.fin_col0, l.fin_ncols, c->nsplit};
    if (c->precise) {
        if (sgn) hipLaunchKernelGGL((k_dot<true, true>), grid, block, c->dot_lds, st, Xp, c->ld, r32, r64, c->nchunks, 1, part, c->m_pad, sy, uq);
        else     hipLaunchKernelGGL((k_dot<true, false>), grid, block, c->dot_lds, st, Xp, c->ld, r32, r64, c->nchunks, 1, part, c->m_pad, sy, uq);
    } else {
        if (sgn) hipLaunchKernelGGL((k_dot<false, true>), grid, block, c->dot_lds, st, Xp, c->ld, r32, r64, c->nchunks, 1, part, c->m_pad, sy, uq);
        else     hipLaunchKernelGGL((k_dot<false, false>), grid, block, c->dot_lds, st, Xp, c->ld, r32, r64, c->nchunks, 1, part, c->m_pad, sy, uq);
    }
    return HB_OK;
}

// digit-plane sums of [col0, col0 + ncols) -> doubles at out (the finalize that has no later launch to ride on)
static void launch_dotq_fin(hb_ctx *c, int col0, int ncols, int gidx, double *out, hipStream_t st)
{
    hipLaunchKernelGGL(k_dotq_fin, dim3((ncols + 63) / 64), dim3(64), 0, st, c->accq + col0, (int64_t)c->m_pad, ncols, c->gexp + gidx, out);
}

// sweep start of the fixed-point path: digits of residual slot 0, bound mb[0], zeroed plane sums
static void launch_quant0(hb_ctx *c, hipStream_t st)
{
    (void)hipMemsetAsync(c->accq, 0, sizeof(long long) * (size_t)HB_ND * c->m_pad, st);
    const int qb = (int)std::max<int64_t>(1, std::min<int64_t>(64, (c->ld / 4 + 255) / 256));
    (void)hipMemsetAsync(c->mb, 0, sizeof(double), st);
    hipLaunchKernelGGL(k_absmax, dim3(qb), dim3(256), 0, st, c->r, c->ld, reinterpret_cast<unsigned long long *>(c->mb));
    hipLaunchKernelGGL(k_quant0, dim3(qb), dim3(256), 0, st, c->r, c->ld, c->rq, c->mb, c->vexp, (const double *)c->mb);
    if (c->row_reduce) { // the shards' maxima -> one exponent for all (host round trip: this is the cross-check mode)
        (void)hipStreamSynchronize(st);
        std::vector<double> slot((size_t)std::max(1, c->row_world), 0.0);
        double mxl = 0.0;
        (void)hipMemcpy(&mxl, c->mb, sizeof(double), hipMemcpyDeviceToHost);
        slot[c->row_rank] = mxl;
        if (c->row_reduce(c->row_user, slot.data(), slot.size())) { c->row_failed = true; return; }
        for (double v : slot) mxl = std::max(mxl, v);
        (void)hipMemcpy(c->scratch, &mxl, sizeof(double), hipMemcpyHostToDevice);
        hipLaunchKernelGGL(k_quant0, dim3(qb), dim3(256), 0, st, c->r, c->ld, c->rq, c->mb, c->vexp, (const double *)c->scratch);
    }
}

// row-sharded cross-check mode: the digit-plane sums of columns [col0, col0 + ncols) summed over the shards (exact: integers
// below 2^53 travel as doubles), before they are finalized
static int row_reduce_accq(hb_ctx *c, int col0, int ncols, hipStream_t st)
{
    HB_HIP(hipStreamSynchronize(st));
    std::vector<long long> hq((size_t)HB_ND * ncols);
    HB_HIP(hipMemcpy2D(hq.data(), sizeof(long long) * ncols, c->accq + col0, sizeof(long long) * c->m_pad, sizeof(long long) * ncols, HB_ND, hipMemcpyDeviceToHost));
    std::vector<double> hd(hq.size());
    for (size_t i = 0; i < hq.size(); i++) hd[i] = (double)hq[i];
    if (c->row_reduce(c->row_user, hd.data(), hd.size())) return hb_fail(HB_ERR_COMM, "row-sharded mode: the all-reduce of the digit sums failed");
    for (size_t i = 0; i < hq.size(); i++) hq[i] = (long long)hd[i];
    HB_HIP(hipMemcpy2D(c->accq + col0, sizeof(long long) * c->m_pad, hq.data(), sizeof(long long) * ncols, sizeof(long long) * ncols, HB_ND, hipMemcpyHostToDevice));
    return HB_OK;
}

// the reduction of the last launch's partials (there is no next launch to carry it)
static void launch_reduce(hb_ctx *c, int col0, int ncols, hipStream_t st, int gidx = 0)
{
    if (fixed_point(c)) {
        launch_dotq_fin(c, col0, ncols, gidx, c->dsum + col0, st);
        return;
    }
    dot_sync sy{c->partial + col0, c->dsum + col0, ncols, c->nsplit};
    hipLaunchKernelGGL(k_reduce_partials, dim3((ncols + 255) / 256), dim3(256), 0, st, sy, c->m_pad);
}

// mbi: index of the group (pipeline) or panel (serial kernels) whose moves are applied — addresses the chain's bound mb[1 + mbi]
static upd_view make_upd(hb_ctx *c, int p0, int p1, int sin, int sout, unsigned *flags, int mbi)
{
    const bool fx = c->precise == 2;
    return upd_view{c->X, c->P, p0, p1, c->ev_count, c->ev_idx, c->ev_delta, c->r + (size_t)sin * c->ld,
                    c->r + (size_t)sout * c->ld, c->u, c->r32 + (size_t)sout * c->ld, flags,
                    fx ? c->rq + (size_t)sout * HB_ND * c->ld : nullptr, c->mb + (size_t)(1 + mbi) * HB_MBS, c->vexp + sout,
                    c->layout == 2 ? c->X2 : nullptr, c->ld2 / 4, 0, c->ddense};
}

struct phase_timer {
    hb_ctx *c;
    bool on;
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> spans;
    size_t next = 0;
    phase_timer(hb_ctx *ctx, bool enable) : c(ctx), on(enable) {}
    hipEvent_t get()
    {
        if (next == c->ev_pool.size()) {
            hipEvent_t e;
            (void)hipEventCreate(&e);
            c->ev_pool.push_back(e);
        }
        return c->ev_pool[next++];
    }
    hipEvent_t begin()
    {
        if (!on) return nullptr;
        hipEvent_t e = get();
        (void)hipEventRecord(e, c->stream);
        return e;
    }
    void end(int phase, hipEvent_t b)
    {
        if (!on) return;
        hipEvent_t e = get();
        (void)hipEventRecord(e, c->stream);
        spans.push_back({phase, {b, e}});
    }
};

// Enqueue one whole sweep (parameters already in c->d_in).
//
// Pipeline (look-ahead L panels).  Three streams; panel p's kernels and their dependencies:
//   A  mat-vec(p)   reads residual version p-L-1                 after update(p-L-1)
//   B  chain(p)     folds in the moves of panels p-L..p-1        after mat-vec(p) and chain(p-1)
//   C  update(p)    residual version p-1 -> p                     after chain(p) and update(p-1)
// so the serial chain of panel p runs while the mat-vecs of the next panels stream from HBM.  Version v
// of the residual lives in slot (v+1) mod (L+1); update(p) overwrites the slot mat-vec(p) has just read.
// `timed` serialises everything on stream A with HIP events around each kernel (same kernels, same results).
static int enqueue_sweep_kernels(hb_ctx *c, int model, int n_fold, bool timed)
{
    phase_timer tm(c, timed);
    const int kp = kpad_for(model, n_fold);
    const int L = c->Lv, np = c->npanels; // per-panel launches: lag Lv with one panel per mat-vec
    hipStream_t sA = c->stream, sB = timed ? c->stream : c->s_chain, sC = timed ? c->stream : c->s_upd;
    // (not a memset: the second sweep of a context, which replays the captured graph, came back with a 16-byte pattern of non-zero denormals in
    // the sums no kernel adds to — class counts past the model's classes, tests/test_gpu_real_sweep.py — and so under every sum that one does)
    hipLaunchKernelGGL(k_zero_acc, dim3(1), dim3(64), 0, sA, c->acc);
    const bool fx = fixed_point(c);
    const bool real = c->layout == 64; // fp64 columns (hb_real.hip): k_dot_real, k_chain on the fp64 Gram block, k_update_real
    if (real && (L != 0 || c->NB != 1 || !c->gramd)) return hb_fail(HB_ERR_INVALID, "the fp64 resident layout runs at lag 0 on its own Gram blocks (hb_ctx_build_gram)");
    if (fx) launch_quant0(c, sA);
    hipEvent_t t_all = tm.begin();
    {
        hipEvent_t b = tm.begin();
        pre_view pv{c->m, c->m_pad, c->m_offset, c->seed, c->xpx, c->vx, c->g, c->vargL, c->thr, c->invv, c->sdz, kp};
        hipLaunchKernelGGL(k_pre, dim3((c->m_pad + 255) / 256), dim3(256), 0, sA, c->d_in, pv);
        tm.end(3, b);
    }
    if (!timed) { // fork the chain and update streams off stream A
        HB_HIP(hipEventRecord(c->ev_fork, sA));
        HB_HIP(hipStreamWaitEvent(sB, c->ev_fork, 0));
        HB_HIP(hipStreamWaitEvent(sC, c->ev_fork, 0));
    }
    const double xabs = std::max(std::abs((double)c->xmin), std::abs((double)c->xmax));
    chain_view cv{c->m_pad, c->P, fx ? 1 : c->nsplit, L, c->Lg, c->xpx, c->vx, c->g, c->tracker, c->nzrate, c->alpha_sum, c->alpha_sq,
                  c->thr, c->invv, c->sdz, real ? reinterpret_cast<const int32_t *>(c->gramd) : c->gram, c->partial, c->dsum, c->ev_count, c->ev_idx, c->ev_delta, c->acc,
                  c->wind, c->wflag, c->dbg, fx ? c->mb : nullptr, xabs};
    if (real) cv.Lb = 0; // (one block per panel)
    const int upd_blocks = (int)((c->ld / 4 + 255) / 256);
    // software pipeline in issue order: mat-vec runs L panels ahead of chain/update in program order too,
    // so that a plain in-order replay of the captured graph is still dependency-correct
    for (int step = 0; step < np + L; step++) {
        const int pd = step;     // panel whose mat-vec is issued now
        const int pc = step - L; // panel whose chain + update are issued now
        if (pd < np) {
            hipEvent_t b = tm.begin();
            const int vread = pd - L - 1;
            if (!timed && vread >= 0) HB_HIP(hipStreamWaitEvent(sA, c->ev_upd[vread], 0));
            dot_launch dl{pd * c->P, c->P, ver_slot(c, vread < -1 ? -1 : vread), sA, pd};
            if (int rc = launch_dot(c, dl)) return rc;
            if (fx && c->row_reduce)
                if (int rcr = row_reduce_accq(c, pd * c->P, c->P, sA)) return rcr;
            if (fx) launch_dotq_fin(c, pd * c->P, c->P, pd, c->partial + (size_t)pd * c->P, sA); // the chain sums one "split"
            if (!timed) HB_HIP(hipEventRecord(c->ev_dot[pd], sA));
            tm.end(0, b);
        }
        if (pc >= 0) {
            hipEvent_t b = tm.begin();
            if (!timed) HB_HIP(hipStreamWaitEvent(sB, c->ev_dot[pc], 0));
            hipError_t e = kp == 1 ? launch_chain<1>(c, cv, pc, sB) : kp == 3 ? launch_chain<3>(c, cv, pc, sB) : launch_chain<7>(c, cv, pc, sB);
            if (e != hipSuccess) return hb_fail(HB_ERR_HIP, std::string("k_chain launch: ") + hipGetErrorString(e));
            if (!timed) HB_HIP(hipEventRecord(c->ev_chain[pc], sB));
            tm.end(1, b);
            b = tm.begin();
            if (!timed) HB_HIP(hipStreamWaitEvent(sC, c->ev_chain[pc], 0));
            const int sin = ver_slot(c, pc - 1), sout = ver_slot(c, pc);
            if (real) { // (lag 0: one residual version, updated in place)
                if (int rc = hbk_real_update(c, pc, c->r + (size_t)sout * c->ld, c->r32 + (size_t)sout * c->ld, sC)) return rc;
            } else
            hipLaunchKernelGGL(k_update, dim3(upd_blocks), dim3(256), 0, sC, c->ld, make_upd(c, pc, pc + 1, sin, sout, nullptr, pc));
            if (!timed) HB_HIP(hipEventRecord(c->ev_upd[pc], sC));
            tm.end(2, b);
        }
    }
    if (!timed) { // join
        HB_HIP(hipStreamWaitEvent(sA, c->ev_upd[np - 1], 0));
        HB_HIP(hipStreamWaitEvent(sA, c->ev_chain[np - 1], 0));
    }
    {
        hipEvent_t b = tm.begin();
        const int sfin = ver_slot(c, np - 1);
        if (sfin != 0) { // the residual between sweeps lives in slot 0
            HB_HIP(hipMemcpyAsync(c->r, c->r + (size_t)sfin * c->ld, sizeof(double) * c->ld, hipMemcpyDeviceToDevice, sA));
            HB_HIP(hipMemcpyAsync(c->r32, c->r32 + (size_t)sfin * c->ld, sizeof(float) * c->ld, hipMemcpyDeviceToDevice, sA));
        }
        if (model == 5) {
            hipLaunchKernelGGL(k_bayesl_post, dim3((c->m + 255) / 256), dim3(256), 0, sA, c->d_in, c->m,
                               c->m_offset, c->seed, c->vx, c->g, c->vargL, 0);
            hipLaunchKernelGGL(k_sum_vec, dim3(1), dim3(1024), 0, sA, c->vargL, c->m, c->acc + HB_ACC_SUMVARGL);
        }
        hipLaunchKernelGGL(k_reduce_ru, dim3(16), dim3(64), 0, sA, c->r, c->u, c->n, c->acc, c->ru_ws, c->flags);
        tm.end(3, b);
    }
    tm.end(4, t_all);
    HB_HIP(hipGetLastError());
    if (timed) {
        HB_HIP(hipStreamSynchronize(c->stream));
        hb_sweep_timing T{};
        for (auto &sp : tm.spans) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, sp.second.first, sp.second.second);
            switch (sp.first) {
            case 0: T.dot_ms += ms; T.dot_launches++; break;
            case 1: T.chain_ms += ms; break;
            case 2: T.update_ms += ms; break;
            case 3: T.other_ms += ms; break;
            case 4: T.total_ms += ms; break;
            }
        }
        c->timing = T;
    }
    return HB_OK;
}

// debug hook (hb_ctx_debug_inject_abort): raise the abort flag once the chain has published `panel` panels — what a waiter that
// timed out does — so that the tests can show a replayed sweep to be the same chain
__global__ void k_inject_abort(unsigned *flags, unsigned panel)
{
    const unsigned long long t0 = wall_clock64();
    while (ld_flag(flags + HB_FLAG_CHAIN_DONE) < panel && !ld_flag(flags + HB_FLAG_ABORT) && wall_clock64() - t0 < HB_TIMEOUT_TICKS)
        __builtin_amdgcn_s_sleep(32);
    st_flag(flags + HB_FLAG_ABORT, 1u);
}

// Persistent pipeline: stream A = mat-vec launches (each also carrying an update row and a partial-sum row),
// stream B = ONE chain workgroup for the whole sweep.  Device-side hand-offs: mat-vec -> chain through dsum[]
// (NaN-prefilled, written through by the partial-sum row of the next launch); chain -> update through
// chain_done; update -> mat-vec is a kernel boundary on stream A.
// The panels [pb, pe) of a sweep (pb a multiple of D): the whole sweep, or one block of a sweep whose shards exchange their
// residual deltas every few mat-vec groups (hb_ctx_sweep_range). A range is self-contained: the residual holds every earlier
// move when it starts, so its corrections start from zero and its version ring from slot 0. `first` also prepares the
// per-sweep data (k_pre, k_hotlist, zeroed sums), `last` closes the sweep (BayesL's variances, the residual's sums).
// env_alone: HB_CHAIN_ALONE, read once per sweep by hb_sweep_enqueue.
// the rows of the chain's row cache k_hotlist lays its lists out for
static int hotlist_nslot(const hb_ctx *c, int kp) { return std::max(0, persist_nslot(c->P, std::min(c->L, HB_LBMAX), kp)); }

static int enqueue_sweep_pipeline(hb_ctx *c, int model, int n_fold, int pb, int pe, bool first, bool last, bool env_alone)
{
    const int kp = kpad_for(model, n_fold);
    const int np = pe, D = c->D, Lv = c->Lv;
    const int g0 = pb / D;                             // absolute index of the range's first mat-vec group
    const int ngroups = (np - pb + D - 1) / D;         // groups in the range
    hipStream_t sA = c->stream, sB = c->s_chain;
    // HB_CHAIN_ALONE=1 / hb_ctx_set_profiling(c, 4) — a TIMING AND COUNTER DIAGNOSTIC, results are meaningless (it needs no
    // co-resident kernels, so it is also how k_chain_persist runs under a counter-collecting profiler, tools/chain_counters.py): the mat-vec launches run first against a pre-set
    // chain_done (their update rows find empty event lists), the chain afterwards with the device to itself; the stamped span
    // (tools/chain_timeline.py with CT_ALONE=1) is then what the chain costs without the mat-vec's memory traffic beside it.
    const bool alone = c->chain_alone || env_alone;
    const bool cert = c->gcert_ok && c->gcmax != nullptr; // (the group chain's certified violation check)
    // WHAT runs — the chain's instantiation, k_fwd and the warmers beside it — is the plan's; from here on only WHEN
    const hb_sweep_plan plan = plan_sweep({model, n_fold, c->P, Lv, D, c->L, cert, c->chain_alone, env_alone, np - pb > 2, c->s_warm != nullptr});
    if (!plan.ok)
        return hb_fail(HB_ERR_UNSUPPORTED, "three groups of seven panels of look-ahead, or two of eight, need the group chain with k_fwd (panel 512; seven: BayesB / BayesC "
                                           "and BayesR with up to four classes; eight: BayesB / BayesC with the certificate)");
    const bool dense = plan.chain == HB_CHAIN_DENSE; // k_chain_dense + k_fold_dense (hb_chain_dense.hpp)
    // sweep start: one kernel clears the sweep sums, the flag block, the event counts (quiet panels do not write theirs) and
    // fills dsum[] with "not written yet" (a NaN no sum can produce); the residual's digit planes are then written (k_quant0,
    // one workgroup) beside k_pre / k_hotlist, which need all the other compute units. The chain must be launched BEFORE the
    // first mat-vec launch (it needs a compute unit with all of its LDS free, and back-to-back mat-vec launches never leave
    // one), so both branches start together after the join.
    const bool dense_upd = dense && c->dense_upd;
    if (c->ldiag) HB_HIP(hipMemsetAsync(c->ldiag, 0, sizeof(unsigned long long) * 4 * ((size_t)c->npanels + 2), sA));
    hipLaunchKernelGGL(k_sweep_init, dim3(256), dim3(256), 0, sA, first ? c->acc : nullptr, c->flags, c->ev_count, c->npanels,
                       reinterpret_cast<unsigned long long *>(c->dsum), c->m_pad, pb, reinterpret_cast<unsigned long long *>(c->fcorr),
                       dense ? reinterpret_cast<unsigned long long *>(c->ddense) : nullptr,
                       c->precise == 2 ? reinterpret_cast<unsigned long long *>(c->mb) : nullptr, 1 + pb / c->D, c->npanels + 2,
                       dense ? reinterpret_cast<unsigned long long *>(c->fcorr2) : nullptr, c->ev_idx,
                       reinterpret_cast<unsigned long long *>(c->ev_delta), c->P);
    const bool fx = c->precise == 2;
    if (fx) {
        HB_HIP(hipEventRecord(c->ev_dot[0], sA));
        HB_HIP(hipStreamWaitEvent(sB, c->ev_dot[0], 0));
        launch_quant0(c, sB);
        HB_HIP(hipEventRecord(c->ev_upd[1 % c->npanels], sB));
    }
    if (first) {
        pre_view pvw{c->m, c->m_pad, c->m_offset, c->seed, c->xpx, c->vx, c->g, c->vargL, c->thr, c->invv, c->sdz, kp};
        hipLaunchKernelGGL(k_pre, dim3((c->m_pad + 255) / 256), dim3(256), 0, sA, c->d_in, pvw);
    }
    // (the per-panel chain is launched with persist_nslot(P, L, kp) below: the same number, since plan_sweep gives a band beyond HB_LBMAX to the
    // group chain only — tests/test_opening_host.py walks the plans for it)
    const int ns = hotlist_nslot(c, kp);
    // (the hot lists are rebuilt for every range: they hold the effects as they are when the range starts)
    hipLaunchKernelGGL(k_hotlist, dim3(c->npanels), dim3(c->P), 0, sA, c->d_in, c->vx, c->g, c->thr, c->xpx, c->kappa, c->P, ns, c->hot_slot,
                       c->hot_list, c->thr0f, c->tracker, (c->gcert_ok && c->gB) ? c->opn : nullptr, c->gB, c->candf);
    if (fx) HB_HIP(hipStreamWaitEvent(sA, c->ev_upd[1 % c->npanels], 0));
    HB_HIP(hipEventRecord(c->ev_fork, sA));
    HB_HIP(hipStreamWaitEvent(sB, c->ev_fork, 0));
    const double xabs = std::max(std::abs((double)c->xmin), std::abs((double)c->xmax));
    chain_view cv{c->m_pad, c->P, c->nsplit, Lv, c->Lg, c->xpx, c->vx, c->g, c->tracker, c->nzrate, c->alpha_sum, c->alpha_sq,
                  c->thr, c->invv, c->sdz, c->gram, c->partial, c->dsum, c->ev_count, c->ev_idx, c->ev_delta, c->acc,
                  c->wind, c->wflag, c->dbg, fx ? c->mb : nullptr, xabs};
    if (cert) { cv.ga = c->ga; cv.gB = c->gB; cv.gcmax = c->gcmax; }
    const int last_panels = np - (g0 + ngroups - 1) * D;
    persist_view pv{np, D, Lv, c->L, c->Lg, pb, c->flags,
                    c->hot_slot, c->hot_list, c->thr0f, c->candf, nullptr, nullptr};
    if (cert) pv.opn = c->opn; // (k_hotlist wrote it: gcert_ok)
    if (plan.fcorr) pv.fcorr = c->fcorr;
    auto launch_the_chain = [&](hipStream_t st) -> int {
        const char *what = dense ? "k_chain_dense" : plan.chain == HB_CHAIN_GROUP ? "k_chain_group" : "k_chain_persist";
        auto launch = [&](const auto &table, int threads, auto... more) -> int { // (the plan's instantiation, with the arguments its family adds)
            const auto *k = find_kernel(table, plan.ct, what);
            if (!k) return HB_ERR_INVALID;
            hipLaunchKernelGGL(k->fn, dim3(1), dim3(threads), persist_smem(c->P), st, c->d_in, cv, pv, more...);
            hipError_t e = hipGetLastError();
            return e == hipSuccess ? HB_OK : hb_fail(HB_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
        };
        if (dense) return launch(dense_chains, 512, c->ddense, c->fcorr2);
        if (plan.chain == HB_CHAIN_GROUP) return launch(group_chains, c->P);
        return launch(persist_chains, c->P, persist_nslot(c->P, c->L, kp));
    };
    if (alone) { // (the update rows poll the move counts themselves: "no moves" for every panel)
        HB_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->flags + HB_FLAG_CHAIN_DONE), 0x7ffffff0, 1, sA));
        HB_HIP(hipMemsetAsync(c->ev_count, 0, sizeof(int32_t) * (size_t)c->npanels * HB_EVS, sA));
        if (fx) HB_HIP(hipMemsetAsync(c->mb + HB_MBS, 0, sizeof(double) * ((size_t)c->npanels + 1) * HB_MBS, sA));
    }
    else {
        // round 6: k_fold_dense is enqueued BEFORE the chain and the gate. Captured after them, the graph started it ~1 ms late — the dense chain waits for its
        // first far sums at sub-block 4 of the sweep's first panel, launch 2's update rows wait for the chain: 1 ms of every 18 ms sweep
        // (tools/r6_long_launch.py, tools/r6_dense_start.py)
        // (Lb + 1 target panels are open at any time: Lb ahead for their band, the chain's own for its far sub-blocks)
        if (dense) {
            HB_HIP(hipStreamWaitEvent(c->s_upd, c->ev_fork, 0));
            hipLaunchKernelGGL(k_fold_dense, dim3(8 * (c->L + 1)), dim3(256), 0, c->s_upd, cv, pv, c->ddense, c->fcorr2, c->L + 1);
            HB_HIP(hipGetLastError());
        }
        if (int rc = launch_the_chain(sB)) return rc;
        // (the first mat-vec launch starts when the chain is resident — where a launch's update blocks can sit on every compute unit)
        if (dense) hipLaunchKernelGGL(k_gate, dim3(1), dim3(64), 0, sA, c->flags);
    }
    if (plan.fwd[0]) { // k_fwd: a second persistent workgroup, on the update stream
        auto *k = find_kernel(fwd_kernels, plan.fwd, "k_fwd");
        if (!k) return HB_ERR_INVALID;
        HB_HIP(hipStreamWaitEvent(c->s_upd, c->ev_fork, 0));
        hipLaunchKernelGGL(k->fn, dim3(1), dim3(c->P), 0, c->s_upd, cv, pv);
        HB_HIP(hipGetLastError());
    }
    if (plan.warm) { // the L2 warmers (k_warm, hb_warm.hpp): a third branch of the graph
        HB_HIP(hipStreamWaitEvent(c->s_upd, c->ev_fork, 0));
        hipLaunchKernelGGL(k_warm, dim3(8 * plan.warm), dim3(256), 0, c->s_upd, pv, cv, kp, c->gram, c->P, plan.warm_ahead, plan.warm, reinterpret_cast<int *>(c->flags + 48));
        HB_HIP(hipGetLastError());
    }
    if (plan.warm_r) { // ... or a fourth, where k_fwd has the third
        HB_HIP(hipStreamWaitEvent(c->s_warm, c->ev_fork, 0));
        persist_view pw = pv;
        pw.Lb = plan.warm_r_Lb;
        hipLaunchKernelGGL(k_warm, dim3(8 * plan.warm_r), dim3(256), 0, c->s_warm, pw, cv, kp, c->gram, c->P, plan.warm_r_ahead, plan.warm_r, reinterpret_cast<int *>(c->flags + 48));
        HB_HIP(hipGetLastError());
    }
    const bool inject = c->inject_abort_panel >= 0 && c->s_dbg && !alone;
    if (inject) { // (debug hook: a fourth branch that aborts the sweep in mid-flight)
        HB_HIP(hipStreamWaitEvent(c->s_dbg, c->ev_fork, 0));
        hipLaunchKernelGGL(k_inject_abort, dim3(1), dim3(1), 0, c->s_dbg, c->flags, (unsigned)std::min(c->inject_abort_panel, np));
        HB_HIP(hipGetLastError());
    }
    const int upd_blocks = (int)((c->ld / 4 + 255) / 256);
    // Residual versions advance per mat-vec group: version h = every panel of groups <= h applied. Mat-vec launch g
    // reads version g - Lv - 1 and, in one extra grid row, carries update(h = g - Lv): version h-1 -> h, which the
    // NEXT launch reads. Two buffers ping-pong (slot = (version + 1) & 1). No third stream, no cross-stream events.
    auto slot2 = [](int v) { return v < 0 ? 0 : ((v + 1) & 1); };
    // (g, h: group indices within the range — they drive the version slots; ga, ha: the absolute ones — they address panels)
    for (int g = 0; g < ngroups; g++) {
        const int ga = g0 + g;
        const int p0 = ga * D, p1 = std::min(np, p0 + D);
        const int h = g - Lv, ha = g0 + h;
        upd_view uq{};
        if (h >= 0) uq = make_upd(c, ha * D, std::min(np, ha * D + D), slot2(h - 1), slot2(h), c->flags, ha);
        uq.dense = (dense_upd && fx && c->layout == 8 && D <= 2) ? 1 : 0; // (one row per lane where every marker moved; the fixed-point mat-vec's single-wave update blocks)
        bool ride = h >= 0;
        if (h >= 0 && dense_upd && !fx && c->layout == 8 && D <= 2) {
            // fp32 / fp64 mat-vec (k_dot: 256-thread blocks): the dense update as its own kernel AHEAD of the launch instead of a
            // grid row in it (11.5 sweeps/s with the fused row at n = 50k, m = 500k). It writes the slot the previous launch read
            // and this launch does not touch.
            uq.dense = 1;
            hipLaunchKernelGGL(k_update_dense, dim3((unsigned)(c->ld / 64)), dim3(64), 0, sA, c->ld, uq);
            ride = false;
        }
        dot_launch dl{p0 * c->P, (p1 - p0) * c->P, slot2(g - Lv - 1), sA, ga};
        if (ride) dl.upd = &uq;
        if (g > 0) dl.fin_col0 = (ga - 1) * D * c->P, dl.fin_ncols = D * c->P;
        if (int rc = launch_dot(c, dl)) return rc;
    }
    launch_reduce(c, (g0 + ngroups - 1) * D * c->P, last_panels * c->P, sA, g0 + ngroups - 1);
    if (alone)
        if (int rc = launch_the_chain(sA)) return rc;
    for (int h = std::max(0, ngroups - Lv); h < ngroups; h++) { // the updates that had no later mat-vec to ride on
        upd_view uq = make_upd(c, (g0 + h) * D, std::min(np, (g0 + h) * D + D), slot2(h - 1), slot2(h), c->flags, g0 + h);
        if (dense_upd && c->layout == 8 && D <= 2) {
            uq.dense = 1;
            hipLaunchKernelGGL(k_update_dense, dim3((unsigned)(c->ld / 64)), dim3(64), 0, sA, c->ld, uq);
        } else hipLaunchKernelGGL(k_update, dim3(upd_blocks), dim3(256), 0, sA, c->ld, uq);
    }
    HB_HIP(hipEventRecord(c->ev_chain[0], sB));
    HB_HIP(hipStreamWaitEvent(sA, c->ev_chain[0], 0));
    if (plan.warm || plan.fwd[0] || dense) {
        HB_HIP(hipEventRecord(c->ev_upd[0], c->s_upd));
        HB_HIP(hipStreamWaitEvent(sA, c->ev_upd[0], 0));
    }
    if (plan.warm_r) {
        HB_HIP(hipEventRecord(c->ev_chain[1 % c->npanels], c->s_warm));
        HB_HIP(hipStreamWaitEvent(sA, c->ev_chain[1 % c->npanels], 0));
    }
    if (inject) {
        HB_HIP(hipEventRecord(c->ev_dot[0], c->s_dbg));
        HB_HIP(hipStreamWaitEvent(sA, c->ev_dot[0], 0));
    }
    const int sfin = slot2(ngroups - 1);
    if (sfin != 0) {
        HB_HIP(hipMemcpyAsync(c->r, c->r + (size_t)sfin * c->ld, sizeof(double) * c->ld, hipMemcpyDeviceToDevice, sA));
        HB_HIP(hipMemcpyAsync(c->r32, c->r32 + (size_t)sfin * c->ld, sizeof(float) * c->ld, hipMemcpyDeviceToDevice, sA));
    }
    if (model == 5 && last) {
        hipLaunchKernelGGL(k_bayesl_post, dim3((c->m + 255) / 256), dim3(256), 0, sA, c->d_in, c->m, c->m_offset, c->seed,
                           c->vx, c->g, c->vargL, 0);
        hipLaunchKernelGGL(k_sum_vec, dim3(1), dim3(1024), 0, sA, c->vargL, c->m, c->acc + HB_ACC_SUMVARGL);
    }
    if (last) hipLaunchKernelGGL(k_reduce_ru, dim3(16), dim3(64), 0, sA, c->r, c->u, c->n, c->acc, c->ru_ws, c->flags);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hb_sweep_enqueue(hb_ctx *c, const hb_sweep_in *in, bool timed)
{
    if (int rc = hbk_set_timeout(c)) return rc;
    *c->h_in = *in;
    HB_HIP(hipMemcpyAsync(c->d_in, c->h_in, sizeof(hb_sweep_in), hipMemcpyHostToDevice, c->stream));
    // (what hb_ctx_debug_get_mirrors reads: the per-panel kernels end in ver_slot(np - 1), a range of the pipeline in slot2(ngroups - 1))
    c->upd_slot = c->npanels % c->NB, c->upd_mbi = c->npanels - 1;
    if (timed || c->row_reduce) return enqueue_sweep_kernels(c, in->model_index, in->n_fold, true); // (row-sharded mode: host round trips inside the sweep)
    const int pb = c->rng_pe ? c->rng_pb : 0, pe = c->rng_pe ? c->rng_pe : c->npanels;
    if (c->pipeline) {
        const int ngroups = (pe - pb + c->D - 1) / c->D;
        c->upd_slot = ngroups & 1, c->upd_mbi = pb / c->D + ngroups - 1;
        // (what hb_ctx_debug_get_opening reports: k_hotlist's arguments in enqueue_sweep_pipeline, whether launched now or replayed from a graph)
        c->hot_ns = hotlist_nslot(c, kpad_for(in->model_index, in->n_fold));
        c->hot_opn = c->gcert_ok && c->gB;
    }
    const bool first = c->rng_pe ? c->rng_first : true, last = c->rng_pe ? c->rng_last : true;
    const bool env_alone = getenv("HB_CHAIN_ALONE") != nullptr; // (tools/chain_timeline.py sets it in the middle of a run)
    auto enqueue = [&]() {
        return c->pipeline ? enqueue_sweep_pipeline(c, in->model_index, in->n_fold, pb, pe, first, last, env_alone)
                           : enqueue_sweep_kernels(c, in->model_index, in->n_fold, false);
    };
    if (c->inject_abort_panel >= 0 && c->pipeline) { // (debug hook: such a sweep is launched directly, never from a cached graph)
        const int rc = enqueue();
        if (last && --c->inject_abort_times <= 0) c->inject_abort_panel = -1;
        return rc;
    }
    if (!c->use_graph) return enqueue();
    if (c->graph_model == -1) { // stale: something the graphs point at has moved
        for (auto &ge : c->gcache) {
            if (ge.e) (void)hipGraphExecDestroy(ge.e);
            if (ge.g) (void)hipGraphDestroy(ge.g);
        }
        c->gcache.clear();
        c->gexec = nullptr;
        c->graph = nullptr;
        c->graph_model = 0;
    }
    c->gexec = nullptr;
    for (auto &ge : c->gcache)
        if (ge.model == in->model_index && ge.fold == in->n_fold && ge.pipeline == c->pipeline && ge.Lv == c->Lv && ge.D == c->D &&
            ge.pb == pb && ge.pe == pe)
            c->gexec = ge.e;
    if (!c->gexec) {
        HB_HIP(hipStreamSynchronize(c->stream));
        HB_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
        int rc = enqueue();
        hipGraph_t g = nullptr;
        hipError_t e = hipStreamEndCapture(c->stream, &g);
        if (rc) return rc;
        if (e != hipSuccess) return hb_fail(HB_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
        hipGraphExec_t ge = nullptr;
        HB_HIP(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        c->gcache.push_back({in->model_index, in->n_fold, c->pipeline, c->Lv, c->D, pb, pe, g, ge});
        c->gexec = ge;
    }
    HB_HIP(hipGraphLaunch(c->gexec, c->stream));
    return HB_OK;
}

// ---- co-residency probe of the persistent pipeline ----
// The pipeline's two graph branches hand-shake through memory (the chain polls dsum[], the update rows poll chain_done), so
// it only makes progress where kernels on two streams really run at the same time. Environments that serialise kernels
// (AMD_SERIALIZE_KERNEL, HIP_LAUNCH_BLOCKING, a counter-collecting profiler, a time-sliced GPU) would stall every sweep
// until its 3 s timeout. The probe: two one-lane kernels on the two streams, each raises its word and waits (<= 10 ms) for the
// other's. Both see each other only if they were co-resident.
__global__ void k_probe(unsigned *w, int me, int other)
{
    st_flag(w + me, 1u);
    const unsigned long long t0 = wall_clock64();
    while (ld_flag(w + other) == 0u) {
        if (wall_clock64() - t0 > 1000000ull) { // 10 ms at 100 MHz
            st_flag(w + me, 2u);
            return;
        }
        __builtin_amdgcn_s_sleep(8);
    }
}

int hbk_probe_concurrency(hb_ctx *c, int *concurrent)
{
    unsigned *w = c->flags + 32;
    HB_HIP(hipMemsetAsync(w, 0, 2 * sizeof(unsigned), c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    hipLaunchKernelGGL(k_probe, dim3(1), dim3(1), 0, c->s_chain, w, 0, 1);
    hipLaunchKernelGGL(k_probe, dim3(1), dim3(1), 0, c->stream, w, 1, 0);
    HB_HIP(hipGetLastError());
    HB_HIP(hipStreamSynchronize(c->s_chain));
    HB_HIP(hipStreamSynchronize(c->stream));
    unsigned h[2] = {0, 0};
    HB_HIP(hipMemcpy(h, w, sizeof(h), hipMemcpyDeviceToHost));
    *concurrent = (h[0] == 1u && h[1] == 1u) ? 1 : 0;
    return HB_OK;
}

// ---- thin launch wrappers used by hb_ctx.cpp ----
int hbk_stats(hb_ctx *c)
{
    if (c->layout == 64) return hbk_real_stats(c);
    int init[2] = {127, -128};
    HB_HIP(hipMemcpyAsync(c->xinfo, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_stats, dim3(c->m_pad), dim3(256), 0, c->stream, c->X, c->ld, c->n, c->m, c->xpx, c->vx, c->xinfo, c->s1);
    HB_HIP(hipGetLastError());
    int info[2];
    HB_HIP(hipMemcpyAsync(info, c->xinfo, sizeof(info), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    c->xmin = info[0];
    c->xmax = info[1];
    c->stats_ready = true;
    return HB_OK;
}

int hbk_dot_all(hb_ctx *c)
{
    if (fixed_point(c)) {
        launch_quant0(c, c->stream);
        for (int p = 0; p < c->npanels; p++) if (int rc = launch_dot(c, dot_launch{p * c->P, c->P})) return rc;
        launch_dotq_fin(c, 0, c->m_pad, 0, c->dots, c->stream);
        HB_HIP(hipGetLastError());
        return HB_OK;
    }
    for (int p = 0; p < c->npanels; p++) if (int rc = launch_dot(c, dot_launch{p * c->P, c->P})) return rc;
    hipLaunchKernelGGL(k_sum_partials, dim3((c->m_pad + 255) / 256), dim3(256), 0, c->stream, c->partial, c->m_pad,
                       c->nsplit, c->m_pad, c->dots);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_dot_panels(hb_ctx *c, int reps)
{
    for (int r = 0; r < reps; r++)
        for (int p = 0; p < c->npanels; p++) if (int rc = launch_dot(c, dot_launch{p * c->P, c->P})) return rc;
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_reduce_ru(hb_ctx *c)
{
    hipLaunchKernelGGL(k_reduce_ru, dim3(16), dim3(64), 0, c->stream, c->r, c->u, c->n, c->acc, c->ru_ws, c->flags);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_shift(hb_ctx *c, double a)
{
    hipLaunchKernelGGL(k_shift, dim3((c->n + 255) / 256), dim3(256), 0, c->stream, c->r, c->r32, c->n, a);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_to_f32(hb_ctx *c)
{
    hipLaunchKernelGGL(k_to_f32, dim3((int)((c->ld + 255) / 256)), dim3(256), 0, c->stream, c->r, c->r32, (int)c->ld);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_cov_dot(hb_ctx *c, int i, double *dev_out)
{
    hipLaunchKernelGGL(k_dot_vec, dim3(1), dim3(1024), 0, c->stream, c->Cmat + (size_t)i * c->n, c->r, c->n, dev_out);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_cov_axpy(hb_ctx *c, int i, double a)
{
    hipLaunchKernelGGL(k_axpy, dim3((c->n + 255) / 256), dim3(256), 0, c->stream, c->r, c->r32, c->Cmat + (size_t)i * c->n, c->n, a);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_level_sums(hb_ctx *c, int term, double *dev_sums, int nlev)
{
    HB_HIP(hipMemsetAsync(dev_sums, 0, sizeof(double) * nlev, c->stream));
    hipLaunchKernelGGL(k_level_sums, dim3((c->n + 255) / 256), dim3(256), 0, c->stream, c->r, c->zid + (size_t)term * c->n, c->n, dev_sums);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_level_axpy(hb_ctx *c, int term, const double *dev_delta)
{
    hipLaunchKernelGGL(k_level_axpy, dim3((c->n + 255) / 256), dim3(256), 0, c->stream, c->r, c->r32, c->zid + (size_t)term * c->n, c->n, dev_delta);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

// ---- snapshot / restore of the state a sweep changes (hb_ctx_snapshot / hb_ctx_restore): every segment in one launch ----
#define HB_SNAP_MAXSEG 12
struct seg_args {
    char *a[HB_SNAP_MAXSEG];       // destination
    const char *b[HB_SNAP_MAXSEG]; // source
    size_t bytes[HB_SNAP_MAXSEG];
};
__global__ __launch_bounds__(256) void k_copy_segs(seg_args s)
{
    const int k = blockIdx.y;
    char *dst = s.a[k];
    const char *src = s.b[k];
    const size_t nb = s.bytes[k], n16 = nb / 16;
    // (every buffer is a device allocation of hb_bufs or a 256-byte aligned offset into one)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x)
        reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(src)[i];
    if (blockIdx.x == 0)
        for (size_t i = n16 * 16 + threadIdx.x; i < nb; i += blockDim.x) dst[i] = src[i];
}

int hbk_copy_segs(hb_ctx *c, const std::vector<hb_ctx::snap_seg> &segs, bool restore)
{
    if (segs.empty()) return HB_OK;
    if (segs.size() > HB_SNAP_MAXSEG) return hb_fail(HB_ERR_INVALID, "hbk_copy_segs: too many segments");
    seg_args s{};
    for (size_t k = 0; k < segs.size(); k++) {
        char *live = static_cast<char *>(segs[k].live), *copy = c->snap + segs[k].off;
        s.a[k] = restore ? live : copy;
        s.b[k] = restore ? copy : live;
        s.bytes[k] = segs[k].bytes;
    }
    hipLaunchKernelGGL(k_copy_segs, dim3(128, (unsigned)segs.size()), dim3(256), 0, c->stream, s);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

// sharded sweep: the rank whose pipeline gave up turns the event count it contributes to the exchange into a NaN, which the
// all-reduce hands to every rank — all of them then restore and replay the sweep together (hb_run::step)
__global__ void k_abort_poison(const unsigned *flags, double *sums)
{
    if (ld_flag(flags + HB_FLAG_ABORT)) sums[HB_ACC_EVENTS] = __longlong_as_double(0x7ff8000000000001ll);
}
int hbk_abort_poison(hb_ctx *c, double *sums)
{
    hipLaunchKernelGGL(k_abort_poison, dim3(1), dim3(1), 0, c->stream, c->flags, sums);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

// The bound is ONE device global per device (every kernel of the module reads it), so two contexts on one device share it: the cache of
// what was uploaded is keyed by the device ordinal and guarded — two host threads driving two contexts must not race on it — and a
// context whose value differs from the device's re-uploads before its sweep. (Contexts on one device that want DIFFERENT bounds at
// the same time get the later one for both: the bound only decides how soon a stalled sweep is given up, never a result.)
int hbk_set_timeout(hb_ctx *c)
{
    static std::mutex mu;
    static std::map<int, int> uploaded_ms;
    const int ms = std::max(1, c->timeout_ms);
    std::lock_guard<std::mutex> lk(mu);
    auto it = uploaded_ms.find(c->device);
    if (it != uploaded_ms.end() && it->second == ms) return HB_OK;
    const unsigned long long ticks = (unsigned long long)ms * 100000ull;
    HB_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(hb_timeout_ticks), &ticks, sizeof ticks, 0, hipMemcpyHostToDevice, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream)); // (the source is a stack word; this happens once per change of the value)
    uploaded_ms[c->device] = ms;
    return HB_OK;
}

int hbk_windows(hb_ctx *c)
{
    if (c->nw) hipLaunchKernelGGL(k_windows, dim3((c->nw + 255) / 256), dim3(256), 0, c->stream, c->wflag, c->wppa, c->nw);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_f64_to_i8(hb_ctx *c, const double *dsrc, int64_t lds, int ncols, int8_t *dst, int *dbad)
{
    const int64_t tot = (int64_t)c->n * ncols;
    hipLaunchKernelGGL(k_f64_to_i8, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, dsrc, lds, c->n, ncols, dst, c->ld, dbad);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_bed_decode(hb_ctx *c, const uint8_t *dbed, int64_t bpc, int nind, const int32_t *drows, int col0, int ncols)
{
    hipLaunchKernelGGL(k_bed_decode, dim3(ncols), dim3(256), 0, c->stream, dbed, bpc, nind, drows, c->n, c->X + (int64_t)col0 * c->ld, c->ld);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_generate(hb_ctx *c, uint64_t seed, int mono_every)
{
    const dim3 grid((unsigned)((c->ld / 4 + 255) / 256), (unsigned)std::min(c->m, 32768));
    hipLaunchKernelGGL(k_generate, grid, dim3(256), 0, c->stream, c->X, c->ld, c->n, c->m, c->m_offset, seed, mono_every);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_delta_pack(hb_ctx *c, const double *r0, const double *u0, double *buf)
{
    hipLaunchKernelGGL(k_delta_pack, dim3((c->n + 255) / 256), dim3(256), 0, c->stream, c->r, c->u, r0, u0, c->n, buf);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_delta_unpack(hb_ctx *c, const double *r0, const double *u0, const double *buf)
{
    hipLaunchKernelGGL(k_delta_unpack, dim3((c->n + 255) / 256), dim3(256), 0, c->stream, c->r, c->u, c->r32, r0, u0, c->n, buf);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_xalpha(hb_ctx *c, const double *dev_alpha, double *dev_out)
{
    HB_HIP(hipMemsetAsync(dev_out, 0, sizeof(double) * (size_t)c->ld, c->stream));
    if (c->layout == 64) return hbk_real_xalpha(c, dev_alpha, dev_out);
    const dim3 grid((unsigned)((c->ld / 4 + 255) / 256), (unsigned)((c->m_pad + 255) / 256));
    hipLaunchKernelGGL(k_xalpha, grid, dim3(256), 0, c->stream, c->X, c->ld, c->layout == 2 ? c->X2 : nullptr, c->ld2 / 4, c->m_pad, dev_alpha, dev_out);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_pack2(hb_ctx *c)
{
    const int64_t ld2w = c->ld2 / 4;
    hipLaunchKernelGGL(k_pack2, dim3((unsigned)(((ld2w + 255) / 256) * c->m_pad)), dim3(256), 0, c->stream, c->X, c->ld, c->X2, ld2w, c->m_pad);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int hbk_unpack2(hb_ctx *c, int col0, int ncols, int8_t *dst)
{
    const int64_t ld2w = c->ld2 / 4;
    hipLaunchKernelGGL(k_unpack2, dim3((unsigned)(((c->ld / 16 + 255) / 256) * (int64_t)ncols)), dim3(256), 0, c->stream,
                       c->X2 + (int64_t)col0 * ld2w, ld2w, dst, c->ld, ncols);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

#include "hb_sbayes.hpp"

// hb_ctx_time_matvec: the panel mat-vec launches of one sweep, as the pipeline issues them (same grouping, same
// partial-sum rows; no update row), back to back on the context's stream between two HIP events
int hbk_time_matvec(hb_ctx *c, int D, int reps, int as_pipeline, double *avg_us, int *launches)
{
    HB_HIP(hipSetDevice(c->device));
    hipEvent_t e0, e1;
    HB_HIP(hipEventCreate(&e0));
    HB_HIP(hipEventCreate(&e1));
    const int ngroups = (c->npanels + D - 1) / D;
    HB_HIP(hipMemsetAsync(c->flags, 0, sizeof(unsigned) * HB_NFLAGS, c->stream));
    if (fixed_point(c)) launch_quant0(c, c->stream);
    // one pass over the sweep's launches, captured into a graph as the sweep itself is (the launches then follow each other
    // as closely as they do in a run), replayed once untimed and `reps` times between the two events
    HB_HIP(hipStreamSynchronize(c->stream));
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    HB_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
    int rc = HB_OK;
    for (int gi = 0; gi < ngroups && !rc; gi++) {
        const int p0 = gi * D, p1 = std::min(c->npanels, p0 + D);
        dot_launch dl{p0 * c->P, (p1 - p0) * c->P};
        dl.gidx = gi;
        if (as_pipeline && gi > 0) dl.fin_col0 = (gi - 1) * D * c->P, dl.fin_ncols = D * c->P;
        rc = launch_dot(c, dl);
    }
    if (as_pipeline) launch_reduce(c, (ngroups - 1) * D * c->P, (c->npanels - (ngroups - 1) * D) * c->P, c->stream, ngroups - 1);
    HB_HIP(hipStreamEndCapture(c->stream, &g));
    if (rc) return rc;
    HB_HIP(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    HB_HIP(hipGraphLaunch(ge, c->stream));
    HB_HIP(hipEventRecord(e0, c->stream));
    for (int r = 0; r < reps; r++) HB_HIP(hipGraphLaunch(ge, c->stream));
    HB_HIP(hipEventRecord(e1, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    float ms = 0;
    HB_HIP(hipEventElapsedTime(&ms, e0, e1));
    *avg_us = (double)ms * 1e3 / ((double)reps * ngroups);
    if (launches) *launches = ngroups;
    (void)hipGraphExecDestroy(ge);
    (void)hipGraphDestroy(g);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return HB_OK;
}

extern "C" int hbk_dot_bench(hb_ctx *c, int D, int reps, int as_pipeline, double *avg_us)
{
    return hbk_time_matvec(c, D, reps, as_pipeline, avg_us, nullptr);
}
