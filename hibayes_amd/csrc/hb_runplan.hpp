// hb_runplan.hpp — the configuration one run gives plan_sweep (hb_plan.hpp): panel, geometry, resident layout, and whether and where the geometry
// follows the regime; and what follows a sweep that aborted. The one statement of these decisions: hb_ctx_create and hb_pipeline_geometry (hb_ctx.hip) and hb_run's set-up and step
// (hb_run.hip) ask here and apply the answer. Pure functions of small integers and booleans, in the order in which a run learns the facts; no
// HIP, no getenv, no hb_ctx: plain g++ -std=c++17, and tests/test_host_logic.py prints every stage against tests/golden/run_plan_table.json
// (the replay's against tests/golden/replay_plan_table.json).
// They are part of the chain's definition: a run on 2-bit genotypes is the int8 run bit for bit only if both take the same geometry in every sweep.
#pragma once
#include "hb_plan.hpp"
#include <cstddef>
#include <cstdint>

// ---- panel ----
// every marker moves (BayesRR / A / L): panels of 512 run k_chain_dense (hb_chain_dense.hpp: static order, the band folded by other compute
// units); small problems keep small panels, whose Gram rows are all LDS-resident in k_chain_persist. What the caller asked for wins.
static inline int plan_panel(int m, bool every_marker_moves, int asked)
{
    if (asked) return asked;
    if (every_marker_moves) return m >= 4096 ? 512 : (m >= 128 ? 128 : 64);
    return m >= 4096 ? 512 : m >= 1024 ? 256 : m >= 256 ? 128 : 64;
}

// ---- geometry ----
struct hb_geometry {
    int pipeline, Lv, D; // the persistent pipeline or the per-panel kernels, mat-vec groups of look-ahead, panels per group
    int L, NB;           // what follows from them: the Gram band in panels, the residual versions in the ring
};

// normalise what was asked for: the persistent pipeline needs co-resident kernels (hbk_probe_concurrency), and the band must be one a chain folds
static inline hb_geometry plan_geometry(bool concurrent, int pipeline, int P, int Lv, int D)
{
    hb_geometry g{};
    g.pipeline = (concurrent && pipeline) ? 1 : 0;
    g.Lv = std::max(0, std::min(6, Lv));
    g.D = g.pipeline ? std::max(1, std::min(8, D)) : 1;
    // Lv counts mat-vec GROUPS of look-ahead; the Gram band then spans (Lv + 1) * D - 1 earlier panels
    const int lbmax = plan_band_limit(P, g.Lv, g.D);
    while ((g.Lv + 1) * g.D - 1 > lbmax) {
        if (g.Lv > 1) g.Lv--; else g.D--;
    }
    g.L = std::max((g.Lv + 1) * g.D - 1, g.Lv);
    g.NB = g.Lv + 1;
    return g;
}

// the geometry a run asks for on a context of its own (wide_lv: 2, or 3 with HB_WIDE_LV=3; no_adaptive_r: HB_NO_ADAPTIVE_R).
// Few markers move per sweep in the point-mass models: long look-ahead, big mat-vec launches; where many or all markers move the forward
// corrections dominate: one panel per launch, two groups of look-ahead (with one, the chain idles for an update + launch boundary per panel)
static inline hb_geometry plan_default_geometry(int model, int n_fold, int P, bool rowmode, int wide_lv, bool no_adaptive_r)
{
    auto ask = [](int pipeline, int Lv, int D) { return hb_geometry{pipeline, Lv, D, 0, 0}; };
    if (rowmode) return ask(0, 0, 1); // per-panel kernels: an exchange sits between each mat-vec and its chain
    // BayesB / C, (2, 7): seven panels per launch, two groups of look-ahead. (Round 5 ran three on the 2-bit layout — 2 % faster then; with round 6's
    // chain it is 2.4 % SLOWER, 445-449 against 456-462 sweeps/s, and its band is 28 blocks instead of 21: HB_WIDE_LV=3 brings it back)
    if (model == 3 || model == 4) return ask(1, wide_lv, 7);
    // k_chain_dense: two panels per launch (45.6 against 39.4 sweeps/s at n=50k, m=500k; (1, 1) 24.8, (1, 2) 27.7)
    if ((model == 1 || model == 2 || model == 5) && P == 512) return ask(1, 2, 2);
    // BayesR with up to four classes: (2, 2) stored, (2, 1) while many markers move (plan_regime)
    if (model == 6 && n_fold <= 4 && P == 512 && !no_adaptive_r) return ask(1, 2, 2);
    return ask(1, 2, 1); // (BayesR with more classes; RR / A / L on small panels: the second group of look-ahead hides the update + launch boundary)
}

// ---- resident layout ----
// 2: the run packs its context's genotypes to 2 bits once the Gram blocks stand; 8: it leaves them as they are (int8 columns on a context of
// its own; a pre-loaded context keeps the layout its owner chose, whatever genotype_bits says). genotype_bits 2 / 8 force a layout, 0 is
// "auto": 2 bits where that is exact AND the faster sweep — codes 0..3 (PLINK's own alphabet, src/read_bed.cpp:116-120), the fixed-point mat-vec,
// and the point-mass models' wide launches (BayesB / BayesC at panel 512: 450 against 213 sweeps/s at n = 50k, m = 500k; the same chain bit for
// bit). The models whose launches cover one or two panels are bound by their chain workgroup and run the lighter int8 kernel beside it — but
// BayesR with up to four classes, measured late in round 6 with k_dotq2m beside both of its chains: 64.5 against 57.8 sweeps/s 300 sweeps after
// a cold start, 102.8 against 98.3 converged — a quarter of the genotype bytes streaming past the chain workgroup's own round trips (round 4's
// "the 2-bit kernel only lengthens the launches" was the v_dot4 kernel). free_bytes is the device's free memory (0 where it cannot be asked).
static inline int plan_layout(int genotype_bits, bool own_ctx, bool rowmode, int precise, int model, int n_fold, int P, int pipeline, int xmin,
                              int xmax, bool no_auto_bits, size_t free_bytes, int m_pad, int64_t ld, int wide_lv)
{
    if (!own_ctx) return 8;
    if (genotype_bits) return genotype_bits == 2 ? 2 : 8;
    const bool sparse_bc = model == 3 || model == 4, mix_r = model == 6 && n_fold <= 4;
    if (rowmode || precise != 2 || !(sparse_bc || mix_r) || P != 512 || !pipeline || xmin < 0 || xmax > 3 || no_auto_bits) return 8;
    // the band of the default geometry — (2, 7): 21 blocks ((3, 7): 28), BayesR's (2, 2): 6 — and the packed genotypes must fit beside the int8
    // columns the band is built from
    const hb_geometry ask = plan_default_geometry(model, n_fold, P, false, wide_lv, false);
    const size_t blocks = (size_t)plan_geometry(true, ask.pipeline, P, ask.Lv, ask.D).L + 1;
    const size_t band = blocks * m_pad * P * sizeof(int32_t), x2 = (size_t)((ld + 511) / 512 * 128) * m_pad;
    return free_bytes > band + x2 + ((size_t)2 << 30) ? 2 : 8;
}

// ---- geometry by regime ----
// While many markers move every move costs one band row per block of the band, so a narrow band wins; once few move, the wide band with its
// big mat-vec launches does (round 3, at n=50k, m=500k: (2,2) 114 vs (2,7) 92 sweeps/s at 3.5 moves per panel, 136 vs 166 at 1.4). The stored
// band serves both; each geometry's captured sweep is cached.
struct hb_regime {
    bool on;                     // choose (Lv, D) per sweep from the previous sweep's moves
    int Lv[2], D[2];             // [0] the wide geometry, [1] the narrow one
    double to_wide, to_narrow;   // moves per panel of the previous sweep below / above which the geometry changes
};

// own_ctx or ctx_adaptive (hb_ctx_set_adaptive): the context is the run's, or its owner asked for it; g: the context's geometry; Lg: the band it stores.
// No rowmode among the inputs: a row-sharded run has put its context on the per-panel kernels by now (g.pipeline == 0), which is off already
static inline hb_regime plan_regime(int model, int n_fold, int P, bool own_ctx, bool ctx_adaptive, const hb_geometry &g, int Lg, bool no_adaptive_r)
{
    const bool may = (own_ctx || ctx_adaptive) && g.pipeline == 1;
    // BayesB / C: only from the wide-band geometry — (2 | 3, 7) or (2, 8) —, whose stored band serves the narrow (2, 2).
    // Round 6, re-measured at n = 50k, m = 500k from a cold start with this round's chains (profiles/r06_regime_bayescpi*.txt; round 3's 2.0 / 2.6 were taken
    // when the wide geometry ran 166 sweeps/s): 2-bit genotypes — at 3.6 moves a panel (2, 2) 148 against (2, 7) 141 sweeps/s, at 2.6: 173 against 189, at
    // 2.1: 187 against 233; int8 columns — at 5.8: 97 against 80, at 3.6: 124 against 131, at 2.6: 131 against 168.
    // One pair of thresholds for both layouts (the geometries cross at 3.2 moves a panel on 2-bit genotypes, at 4.2 on int8 columns): a run on 2-bit
    // genotypes is the int8 run BIT FOR BIT only if both take the same geometry in every sweep (tests/test_gpu_depth.py
    // test_two_bit_resident_layout_is_the_same_chain; per-layout thresholds broke exactly that), and between 3.2 and 4.2 the int8 run loses 5 % for
    // a handful of sweeps.
    if ((model == 3 || model == 4) && may && (((g.Lv == 2 || g.Lv == 3) && g.D == 7) || (g.Lv == 2 && g.D == 8)) && Lg >= 20)
        return hb_regime{true, {g.Lv, 2}, {g.D, 2}, 3.2, 4.0};
    // Round 6, BayesR with up to four classes at panel 512: two panels per launch and the certified group chain (k_chain_group<3, 2, 2, 15> + k_fwd +
    // warmers) once fewer than ~22 markers a panel move, one panel per launch and the per-panel chain with its row cache (k_chain_persist) above ~27
    // (measured at n = 50k, m = 500k from a cold start, profiles/r06_bayesr_regime.txt: they cross at 19 moves per panel — 47.5 sweeps/s both; at 51:
    // 37 against 54; at 11: 68 against 60; at 8: 85 against 69. Re-measured with k_fwd and the warmers beside the group chain,
    // profiles/r06_bayesr_regime2.txt: at 19.6 moves a panel 51.4 against 49.6 sweeps/s, at 11: 78 against 63; at 47: 39 against 54 — no
    // measurement in between)
    if (model == 6 && n_fold <= 4 && P == 512 && may && g.Lv == 2 && g.D == 2 && Lg >= 5 && !no_adaptive_r)
        return hb_regime{true, {2, 2}, {2, 1}, 22.0, 27.0};
    return hb_regime{};
}

// the geometry (0 wide, 1 narrow) of the next sweep, from the one in force and the previous sweep's moves per panel on this shard: a hysteresis
static inline int regime_next(const hb_regime &r, int cur, double moves_per_panel)
{
    if (cur == 1 && moves_per_panel < r.to_wide) return 0;
    if (cur == 0 && moves_per_panel > r.to_narrow) return 1;
    return cur;
}

// ---- replaying an aborted sweep ----
// A sweep whose pipeline gave up waiting (HB_ERR_ABORTED: every wait on the device is bounded) is replayed from the state saved
// before it. hb_run's step() asks here what follows and applies it: snapshot, restore, the switch of geometry, the line on stderr.
struct hb_replay_state {
    int aborts = 0;                    // sweeps replayed so far (hb_bayes_out.sweeps_replayed)
    int win_start = 0, win_count = 0;  // the 64-iteration window: the iteration that opened it, the aborts in it
    int slow_timeout = 0;              // ms; three aborts within a window: a slow device, not a stall — the run's sweeps wait longer from then on
};

// recovery at all: HB_RECOVER not switched off, on the persistent pipeline (the per-panel kernels wait for nothing on the device), individuals not sharded
static inline bool replay_enabled(bool recover_on, int pipeline, bool rowmode) { return recover_on && pipeline && !rowmode; }

// The wait bound a sweep starts with. A sweep that is replayed when it times out may give up early: a healthy hand-off takes microseconds, the
// device's own pauses a millisecond, so 100 ms instead of the context's 3 s — unless HB_TIMEOUT_MS fixed the bound (timeout_env), or the run has
// learnt that this device is slow. Without recovery the context's bound stays.
static inline int replay_first_wait_ms(bool recover, bool timeout_env, int ctx_timeout_ms, const hb_replay_state &s)
{
    return recover && !timeout_env ? std::max(100, s.slow_timeout) : ctx_timeout_ms;
}

struct hb_replay_step {
    bool replay;          // restore and run the sweep again; false: the abort is the run's failure
    bool to_per_panel;    // first switch to the event-ordered per-panel kernels
    int timeout_ms;       // the replay's wait bound
    hb_replay_state state;
};

// What follows the abort of attempt `attempt` (0: the sweep's first try) in iteration `iter`, with the wait bound timeout_ms in force; fell_back: an
// earlier replay of this sweep already switched to the per-panel kernels.
static inline hb_replay_step replay_after_abort(bool recover, int attempt, bool fell_back, int iter, int timeout_ms, const hb_replay_state &s)
{
    if (!recover || attempt >= 3) return hb_replay_step{false, false, timeout_ms, s}; // at most three replays: the fourth failure ends the run
    hb_replay_step d{true, false, timeout_ms, s};
    d.state.aborts++;
    // a second time-out of the same sweep: the per-panel kernels, once
    d.to_per_panel = attempt >= 1 && !fell_back;
    // (the replay waits 3 s: a wait that was merely slow — a shared or profiled GPU — then gets through)
    d.timeout_ms = std::max(timeout_ms, 3000);
    // a run that keeps aborting is on a slow device, not in a stall (those come once in a few thousand sweeps): wait longer from now on
    if (iter - d.state.win_start > 64) { d.state.win_start = iter; d.state.win_count = 0; }
    if (++d.state.win_count >= 3) d.state.slow_timeout = std::min(3000, std::max(100, d.state.slow_timeout) * 4);
    return d;
}
