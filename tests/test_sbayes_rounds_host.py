"""The fixtures of test_gpu_sbayes_rounds.py proved without a GPU: on every case of tests/sbayes_rounds_cases.py the sequential
reference's trace (tests/sbayess_restatement.py, trace=) shows that the regime the case is named for really occurs — crossers,
more than 64 candidates and more than 64 moves in a group, the cascade, the leaver, the group edges, the empty group — that the
matrix is positive definite, that the restatement on the fully stored matrix equals the C oracle of SBayesD() bit for bit with
nothing redrawn (so the one trace is valid for the dense route too), and that the trace changes nothing. What the kernels make of
these inputs is the GPU file's business; nothing here simulates a round."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from sbayess_restatement import sbayess_restatement
import sbayes_rounds_cases as K

BITS = ("s_alpha", "s_Vg", "s_Ve", "s_h2", "s_pi", "r_hat", "g_last", "pip", "alpha", "pi")


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("size"):
        return K.size(int(name[4:]))
    return {"rounds": K.rounds, "everyone": K.everyone, "empty": K.empty_group}[name]()


@functools.lru_cache(maxsize=None)
def traced(name, mname):
    """the restatement on the fully stored matrix with its trace, and what the tests derive from each sweep's record"""
    _, model, Pi, fold = next(x for x in K.ROUNDS_MODELS + K.EVERYONE_MODELS if x[0] == mname)
    c, tr = case(name), []
    r = sbayess_restatement(c["ss"], c["full"], model, Pi, fold=fold, seed=K.SEED, trace=tr, **K.RUN)
    assert len(tr) == 3
    return r, tr, [K.derive(rec) for rec in tr]


def check_pinned(name, mname):
    """positive definite; restatement == C oracle in every bit on forms (i) / (ii), no redraw; trace on == trace off; the chain
    stays where a variance is a variance on the non-zeros' form too"""
    _, model, Pi, fold = next(x for x in K.ROUNDS_MODELS + K.EVERYONE_MODELS if x[0] == mname)
    c = case(name)
    assert np.linalg.eigvalsh(c["dense"]).min() > 0
    assert c["full"].nnz == c["m"] ** 2 and c["nz"].nnz == np.count_nonzero(c["dense"])
    r, tr, _ = traced(name, mname)
    assert r["redraws"] == 0 and r["zeroed"] == 0
    ref = O.sbayes(c["ss"], c["dense"], model, Pi, fold=fold, seed=K.SEED, rng=O.RNG_PHILOX, store_alpha=True, **K.RUN)
    assert r["n_records"] == ref["n_records"] == 3 and r["n"] == ref["n"] == K.N_OBS and r["count_y"] == ref["count_y"] and r["nzct"] == ref["nzct"]
    for k in BITS:
        assert np.array_equal(r[k], ref[k]), k
    off = sbayess_restatement(c["ss"], c["full"], model, Pi, fold=fold, seed=K.SEED, **K.RUN)
    for k in BITS:
        assert np.array_equal(r[k], off[k]), k
    for rec in tr:                                         # the trace is consistent with the records it sits beside
        assert not rec["moved"][np.isnan(c["ss"][:, 1])].any() and not rec["entry_in"][np.isnan(c["ss"][:, 1])].any()
    for s in range(3):
        assert np.array_equal(tr[s]["g_before"], r["s_alpha"][:, s - 1] if s else np.zeros(c["m"]))
        assert np.array_equal(tr[s]["moved"], r["s_alpha"][:, s] != tr[s]["g_before"])
        assert np.array_equal(tr[s]["turn_in"], r["s_alpha"][:, s] != 0)
    nz = sbayess_restatement(c["ss"], c["nz"], model, Pi, fold=fold, seed=K.SEED, trace=[], **K.RUN)
    assert nz["redraws"] == 0 and np.isfinite(nz["s_alpha"]).all() and (nz["s_Vg"] > 0).all() and (nz["s_Ve"] > 0).all()
    nzoff = sbayess_restatement(c["ss"], c["nz"], model, Pi, fold=fold, seed=K.SEED, **K.RUN)
    for k in BITS:
        assert np.array_equal(nz[k], nzoff[k]), k
    return r, nz


@pytest.mark.parametrize("mname", [x[0] for x in K.ROUNDS_MODELS])
def test_rounds_has_every_regime_it_is_named_for(mname):
    c = case("rounds")
    assert c["m"] == 1100 and np.flatnonzero(np.isnan(c["ss"][:, 1])).tolist() == [149, 512, 700]
    r, nz = check_pinned("rounds", mname)
    assert r["count_y"] == 1097
    _, tr, d = traced("rounds", mname)
    d0 = d[0]
    print(mname, "sweep 0: crossers among the 70 second markers %d, per group: candidates at entry %s, crossers %s, moves %s"
          % (d0["crosser"][K.ROUNDS_SECOND].sum(), K.per_group(d0["cand_entry"], 1100), K.per_group(d0["crosser"], 1100), K.per_group(d0["moved"], 1100)))
    # ---- sweep 0 ----
    assert d0["crosser"][K.ROUNDS_SECOND].sum() >= 60
    cand0 = np.flatnonzero(d0["cand_entry"][:K.GS])
    assert cand0.size > K.ROUND and d0["crosser"][:cand0[K.ROUND]].any()      # more than one round, a rollback in the first
    assert d0["crosser"][301] and d0["crosser"][302]                         # the cascade: two rollbacks in a row
    assert tr[0]["turn_in"][300] and tr[0]["entry_in"][300]
    assert d0["crosser"][511] and d0["crosser"][1099]                        # a group's last marker, the ragged tail's last marker
    for j in (1024, 1050):                                                   # pushed in across a group edge: the update kernel did it
        assert tr[0]["entry_in"][j] and not d0["crosser"][j] and tr[0]["turn_in"][j]
    assert d0["leaver"][401] and tr[0]["turn_in"][400]
    assert d0["moved"][:K.GS].sum() > K.ROUND                                # k_sb_update's second chunk of 64
    # ---- sweeps 1 and 2: markers in the model ----
    for s in (1, 2):
        assert (tr[s]["g_before"] != 0).sum() >= 100
        print(mname, "sweep %d: in the model %d, left it %d, crossers %s, per group: candidates at entry %s, moves %s"
              % (s, (tr[s]["g_before"] != 0).sum(), d[s]["left_model"].sum(), np.flatnonzero(d[s]["crosser"]).tolist(),
                 K.per_group(d[s]["cand_entry"], 1100), K.per_group(d[s]["moved"], 1100)))
    assert d[1]["left_model"].any() or d[2]["left_model"].any()
    assert any((d[s]["crosser"] & (tr[s]["g_before"] == 0)).any() for s in (1, 2))
    assert d[1]["crosser"][211] and d[1]["cand_entry"][210] and tr[1]["g_before"][211] == 0      # the cascade with its driver last
    assert d[1]["cand_entry"][:K.GS].sum() > K.ROUND and d[1]["moved"][:K.GS].sum() > K.ROUND
    # ---- the non-zeros' form: varediff is live, and the rows of (150, 1050) skip a group ----
    assert not np.array_equal(nz["s_alpha"], r["s_alpha"]) and (np.diff(c["nz"].indptr) == 1).sum() > 900
    col = c["nz"].indices[c["nz"].indptr[150]:c["nz"].indptr[151]]
    assert col.tolist() == [150, 1050]


@pytest.mark.parametrize("mname", [x[0] for x in K.EVERYONE_MODELS])
def test_everyone_moves_every_marker_in_every_sweep(mname):
    c = case("everyone")
    assert c["m"] == 513 and np.flatnonzero(np.isnan(c["ss"][:, 1])).tolist() == [0, 511]
    check_pinned("everyone", mname)
    _, tr, d = traced("everyone", mname)
    for s in range(3):                                     # eight rounds of 64 candidates and 64 moves, the last of 62
        assert K.per_group(d[s]["moved"], 513) == [510, 1] and K.per_group(d[s]["cand_entry"], 513) == [510, 1]
        assert tr[s]["entry_in"].sum() == 511 and not d[s]["crosser"].any()


@pytest.mark.parametrize("m", K.SIZES)
def test_sizes_around_a_round_and_a_group(m):
    """The last marker is the second of a pair, so it is a crosser in sweep 0 wherever it shares a group with its driver: every m
    >= 2 but 513, where it is the only marker of the second group — there no round can pass over it, and what has to hold
    instead is that the update kernel carried the driver's move (marker 511, the first group's last) over the edge: the marker is
    over its threshold when its group starts. A crosser is by definition not a candidate at entry, so m = 64 has 63 candidates at
    entry in sweep 0 and the crosser makes the repeated round exactly full; m = 65 has 64 and the crosser is the 65th, the first
    of a second round. In sweep 1 every marker is in the model: 64 and 65 candidates at entry."""
    name = "size%d" % m
    c = case(name)
    assert c["m"] == m
    r, _ = check_pinned(name, "cpi")
    _, tr, d = traced(name, "cpi")
    print("m = %d: candidates at entry per sweep %s, moves %s, crossers in sweep 0 %s"
          % (m, [int(x["cand_entry"].sum()) for x in d], [int(x["moved"].sum()) for x in d], np.flatnonzero(d[0]["crosser"]).tolist()))
    if m == 1:
        assert any(rec["turn_in"][0] for rec in tr)
        return
    if m == 513:
        assert tr[0]["turn_in"][511] and tr[0]["entry_in"][512] and tr[0]["turn_in"][512] and not d[0]["crosser"][512]
    else:
        assert d[0]["crosser"][m - 1] and tr[0]["turn_in"][m - 2]
    if m in (64, 65):
        assert d[0]["cand_entry"].sum() == m - 1 and d[0]["moved"].sum() == m
        assert d[1]["cand_entry"].sum() == m and d[1]["moved"].sum() == m


def test_empty_group_between_two_that_move():
    c = case("empty")
    assert c["m"] == 1030 and np.isnan(c["ss"][512:1024, 1]).all() and not np.isnan(c["ss"][:512, 1]).any()
    r, _ = check_pinned("empty", "cpi")
    assert r["count_y"] == 518
    _, tr, d = traced("empty", "cpi")
    for s in range(3):
        mv = K.per_group(d[s]["moved"], 1030)
        assert mv[0] > 0 and mv[1] == 0 and mv[2] > 0
    assert d[0]["crosser"][101] and d[0]["crosser"][1025]
