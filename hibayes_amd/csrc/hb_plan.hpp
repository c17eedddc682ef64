// hb_plan.hpp — which kernels one sweep of the persistent pipeline runs, as a pure function of a handful of small integers. No HIP in here: it
// compiles with plain g++ -std=c++17, and tests/test_host_logic.py prints the plan of every input against tests/golden/sweep_plan_table.json.
// enqueue_sweep_pipeline (hb_kernels.hip) asks once per sweep and decides only WHEN each kernel is enqueued; hb_pipeline_geometry (hb_ctx.hip)
// asks for the band limit. The HB_*_KERNELS lists below are the one list of the instantiations a plan may name: hb_kernels.hip expands them
// into its launch tables, the test into the sets every plan must lie in.
#pragma once
#include <algorithm>
#include <initializer_list>

#define HB_LBMAX 20 /* panels of band k_chain_persist / k_chain_dense fold into */
#ifndef HB_W8_CH
#define HB_W8_CH 3 /* moves per trip of the eight-panel group chain (4 spills nine registers, 3 four) */
#endif

// padded count of non-null mixture classes: BayesR's n_fold - 1, rounded up to 1 / 3 / 7; every other model has one
static inline int kpad_for(int model, int n_fold)
{
    if (model != 6) return 1;
    const int k1 = n_fold - 1;
    return k1 <= 1 ? 1 : (k1 <= 3 ? 3 : 7);
}

// k_chain_group<K1, DM, FW, CH, CERT>: K1 = 3 BayesR with up to four classes, 1 BayesB / BayesC; DM panels per launch at most, FW panels folded ahead,
// CH moves per trip, CERT the certified violation check (panel 512)
#define HB_GROUP_KERNELS(X) X(3, 2, 2, 15, 1) X(3, 8, 7, 4, 1) X(3, 8, 7, 4, 0) X(3, 4, 8, 5, 1) X(3, 8, 14, 3, 0) X(3, 2, 4, 10, 1) X(3, 2, 4, 10, 0) \
    X(1, 8, 8, HB_W8_CH, 1) X(1, 8, 7, 4, 1) X(1, 8, 7, 4, 0) X(1, 8, 14, 3, 0) X(1, 2, 4, 10, 0) X(1, 1, 2, 20, 0)
// k_chain_persist<K1, NPL>: candidate rows ahead (NPL == the band) for the band widths of the default geometries; any other band goes without
#define HB_PERSIST_KERNELS(X) X(1, 20) X(1, 17) X(1, 1) X(1, 0) X(3, 2) X(3, 0) X(7, 2) X(7, 0)
// k_chain_dense<LASSO>: BayesL's step or BayesRR / BayesA's
#define HB_DENSE_KERNELS(X) X(0) X(1)
// k_fwd<D, G, CH>: D panels per group, G groups folded beyond the chain's share, CH moves per trip
#define HB_FWD_KERNELS(X) X(2, 1, 16) X(8, 1, 8) X(7, 1, 8) X(7, 2, 4) X(1, 1, 16) X(1, 2, 8)

struct hb_sweep_shape {
    int model, n_fold; // hb_sweep_in's model_index and n_fold
    int P, Lv, D, L;   // panel, mat-vec groups of look-ahead, panels per group, Gram band (hb_pipeline_geometry)
    bool cert;         // the certificate is usable (gcert_ok and gcmax)
    bool chain_alone;  // hb_ctx_set_profiling bit 2 ...
    bool env_alone;    // ... and HB_CHAIN_ALONE: not interchangeable, the group chain is refused by the first only
    bool long_range;   // the range has more than two panels
    bool warm_stream;  // the warmers' own stream exists
};

enum { HB_CHAIN_PERSIST = 0, HB_CHAIN_GROUP = 1, HB_CHAIN_DENSE = 2 };

struct hb_sweep_plan {
    bool ok;             // false: no kernel folds this band for this model (HB_ERR_UNSUPPORTED)
    int chain;           // HB_CHAIN_*
    int ct[5];           // the chain's template arguments, in the order of its HB_*_KERNELS list (unused ones 0)
    int fwd[3];          // k_fwd beside the chain, on the update stream: its template arguments (fwd[0] == 0: none)
    bool fcorr;          // the chain reads corrections another kernel writes (persist_view.fcorr)
    int warm, warm_ahead;                // k_warm on the update stream: workgroups per XCD (0: none), panels ahead of chain_done
    int warm_r, warm_r_ahead, warm_r_Lb; // k_warm on its own stream: the same, and the band it warms
};

// the widest Gram band a geometry may ask for: 20 is what k_chain_persist folds; 27 with k_fwd beside the group chain at panel 512 — three groups
// of seven panels of look-ahead, or two of eight (23, round 6) — which plan_sweep refuses for the models and certificates that have no such chain
static inline int plan_band_limit(int P, int Lv, int D) { return (P == 512 && ((Lv == 3 && D == 7) || (Lv == 2 && D == 8))) ? 27 : HB_LBMAX; }

static inline hb_sweep_plan plan_sweep(const hb_sweep_shape &s)
{
    hb_sweep_plan p{};
    const int model = s.model, kp = kpad_for(model, s.n_fold), Lv = s.Lv, D = s.D;
    const bool p512 = s.P == 512, cert = s.cert;
    // either switch is a TIMING AND COUNTER DIAGNOSTIC: the mat-vec launches first, the chain afterwards with the device to itself — nothing beside it
    const bool alone = s.chain_alone || s.env_alone;
    // the models in which every marker moves (BayesRR / A / L) at panel 512: k_chain_dense + k_fold_dense (hb_chain_dense.hpp)
    const bool dense = kp == 1 && (model == 1 || model == 2 || model == 5) && p512 && !alone && s.L <= HB_LBMAX;
    // the point-mass models run the group-granular chain (hb_chain_group.hpp) in one of three sizes: 2 one panel per launch, 1 up to two, 0 up to eight.
    // round 6: BayesR with up to four classes (kp == 3) runs it too wherever a launch covers more than one panel. K1 nested thresholds per candidate
    // instead of one; everything else — candidates, certificate (it bounds the right-hand side, not the class), fold, k_fwd — is the point-mass
    // models' path. The other models run k_chain_persist.
    const int size = (D <= 1 && Lv * D <= 2) ? 2 : (D <= 2 && Lv * D <= 4) ? 1 : ((D <= 8 && Lv * D <= 14) || plan_band_limit(s.P, Lv, D) > HB_LBMAX) ? 0 : -1;
    const bool mix = kp == 3 && model == 6 && D >= 2;
    const bool group = !dense && size >= 0 && !s.chain_alone && ((kp == 1 && (model == 3 || model == 4)) || mix);
    // k_fwd beside the wide group chain: the chain folds a move into its own group and the next (15 rows, four moves per trip), a second workgroup
    // into the group after that (Lv = 2) or the two after that (Lv = 3)
    const bool fwd7 = group && (Lv == 2 || Lv == 3) && D == 7 && p512 && !alone;
    // round 6: also beside BayesR's two-panel groups ((2, 2): the chain folds a move into the next group's two panels, k_fwd into the two after — half
    // of the chain's fold rows leave its compute unit, and a group's ~16 moves fit ONE trip of 62 loads per lane instead of two of 60)
    const bool fwd2 = group && mix && Lv == 2 && D == 2 && p512 && !alone && cert;
    // round 6: eight panels per launch (Lv = 2 only, point-mass models, certified): k_chain_group<1, 8, 8, CH, CERT> + k_fwd<8, 1, 8>
    const bool wide8 = group && kp == 1 && Lv == 2 && D == 8 && p512 && !alone && cert;
    if (s.L > HB_LBMAX && !(fwd7 || fwd2 || wide8)) return p;
    p.ok = true;
    // BayesR on the per-panel chain (round 4): k_fwd folds a panel's moves into the panels two (and, at Lv = 3, three) ahead, the chain itself only
    // into the next one — half (two thirds) of the band rows of a dense sweep leave the chain's compute unit
    const bool fwdp = !dense && !group && kp == 3 && p512 && D == 1 && (Lv == 2 || Lv == 3) && !alone && s.long_range;
    // one row per case: the chain's template arguments and, where one runs, k_fwd's
    auto set = [](int *dst, std::initializer_list<int> v) { std::copy(v.begin(), v.end(), dst); };
    const int c512 = cert && p512;
    const bool narrow = D <= 4 && Lv * D <= 8 && size == 0; // three or four panels per launch
    p.chain = dense ? HB_CHAIN_DENSE : group ? HB_CHAIN_GROUP : HB_CHAIN_PERSIST;
    if (dense) set(p.ct, {model == 5});
    else if (fwd2) set(p.ct, {3, 2, 2, 15, 1}), set(p.fwd, {2, 1, 16});
    else if (wide8) set(p.ct, {1, 8, 8, HB_W8_CH, 1}), set(p.fwd, {8, 1, 8});
    else if (fwd7 && Lv == 2) set(p.ct, {kp, 8, 7, 4, c512}), set(p.fwd, {7, 1, 8});
    else if (fwd7) set(p.ct, {kp, 8, 7, 4, c512}), set(p.fwd, {7, 2, 4});
    else if (group && mix && c512 && narrow) set(p.ct, {3, 4, 8, 5, 1});
    else if (group && size == 0) set(p.ct, {kp, 8, 14, 3, 0});
    else if (group && size == 1) set(p.ct, {kp, 2, 4, 10, mix ? c512 : 0});
    else if (group) set(p.ct, {1, 1, 2, 20, 0});
    else if (kp == 1) set(p.ct, {1, (s.L == 20 || s.L == 17 || s.L == 1) ? s.L : 0}); // (candidate rows ahead at the default geometries: 20 is (Lv, D) = (2, 7), 17 (2, 6))
    else if (fwdp && Lv == 2) set(p.ct, {kp, 0}), set(p.fwd, {1, 1, 16}); // (with k_fwd beside it the chain requests its fold rows itself, after the rounds)
    else if (fwdp) set(p.ct, {kp, 0}), set(p.fwd, {1, 2, 8});
    else set(p.ct, {kp, s.L == 2 ? 2 : 0});
    p.fcorr = dense || p.fwd[0] != 0;
    // the L2 warmers (k_warm): a third branch of the graph, four workgroups per XCD of which only the chain's XCD's stay; not beside the group chain
    // and k_fwd, which has the third stream
    constexpr int warm_per_xcd = 4;
    if (!alone && !group && !dense && !fwdp) p.warm = warm_per_xcd, p.warm_ahead = D + 4;
    // BayesR with k_fwd beside the chain: the warmers on a stream of their own. They read the Gram rows of EVERY marker on a panel's hot list, with or
    // without a slot in the chain's row cache, and the rows their moves fold into the next panel (the chain's share of the band). The same beside
    // BayesR's two-panel group chain with k_fwd: the listed markers' Gram rows for the chain's share of the band (its own group and the next: 2 D - 1
    // blocks) and the panels' exact per-marker data (round 6: 92.1 sweeps/s without, 95.9 / 97.5 / 96.5 with 2 / 4 / 8 workgroups per XCD,
    // profiles/r06_bayesr_conv_warm.txt; beside the wide BayesCpi shape: no effect, round 5)
    if ((fwdp || fwd2) && s.warm_stream) {
        p.warm_r = warm_per_xcd;
        // (measured, BayesR at n = 50k, m = 500k: off 48.3 sweeps/s, 2 panels ahead 51.2, 4 ahead 50.5, 8 ahead 50.0)
        p.warm_r_ahead = fwd2 ? 2 * D : 2;
        p.warm_r_Lb = fwd2 ? 2 * D - 1 : 1; // (per panel: the chain folds into the next panel only; the group chain: into its own group's later panels and the next group's)
    }
    return p;
}
