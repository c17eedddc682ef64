"""The control logic of the summary-level chain kernels on the MI355X — k_sb_group / k_sb_update (hb_sbayes.hpp) and k_ss_group /
k_ss_update (hb_sbayes_sparse.hip): the 64-candidate limit of a round, markers a round passed over and pushed over their threshold
(rollback, also twice in a row), the chunked folds, the group edges, a group with nobody to move, the rows' cursor — on the inputs
of tests/sbayes_rounds_cases.py, where test_sbayes_rounds_host.py proves from the sequential reference's trace that each of these
occurs. Three sweeps from g = 0, every sweep recorded and compared with test_gpu_sbayes.py's _compare at the project's tolerances
(inclusion pattern identical, alpha rtol 1e-9, 1e-6 for BayesL):

  dense   H.SBayesD on the ndarray                       against the C oracle O.sbayes;
  full    H.SBayesS on the CSC that stores every entry   against the same (varediff = 0: the two samplers coincide);
  nz      H.SBayesS on the CSC of the non-zeros          against the restatement (varediff live, rows that skip groups).

And beyond _compare: r_hat = xy - n ldm g_last in long double from the device's own g_last to 1e-9 max|xy| (one lost move of a
small effect is far above that, far below _compare's 1e-7 max|r_hat|), and the number of moves the device counted equal to the
trace's — a rolled-back round must not be counted, no move twice."""
import functools

import numpy as np
import pytest

import hibayes_amd as H
from oracle import oracle as O
from sbayess_restatement import sbayess_restatement
import sbayes_rounds_cases as K
from test_gpu_sbayes import _compare
from test_gpu_sbayess import same_run

pytestmark = pytest.mark.gpu
FORMS = ["dense", "full", "nz"]
CASES = ([("rounds",) + x for x in K.ROUNDS_MODELS] + [("everyone",) + x for x in K.EVERYONE_MODELS]
         + [("size%d" % m,) + K.CPI for m in K.SIZES] + [("empty",) + K.CPI])


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("size"):
        return K.size(int(name[4:]))
    return {"rounds": K.rounds, "everyone": K.everyone, "empty": K.empty_group}[name]()


@functools.lru_cache(maxsize=None)
def reference(name, mname, model, sparse):
    """computed once per case and model, shared by the tests and left unchanged: (records, the trace's number of moves)"""
    _, _, Pi, fold = next(x for x in CASES if x[0] == name and x[1] == mname)[1:]
    c, tr = case(name), []
    rs = sbayess_restatement(c["ss"], c["nz" if sparse else "full"], model, Pi, fold=fold, seed=K.SEED, trace=tr, **K.RUN)
    moves = sum(int(rec["moved"].sum()) for rec in tr)
    if sparse:
        return rs, moves
    return O.sbayes(c["ss"], c["dense"], model, Pi, fold=fold, seed=K.SEED, rng=O.RNG_PHILOX, store_alpha=True, **K.RUN), moves


def run(name, form, model, Pi, fold):
    c = case(name)
    kw = dict(fold=fold, seed=K.SEED, verbose=False, **K.RUN)
    if form == "dense":
        return H.SBayesD(c["ss"], c["dense"], model, Pi, **kw)
    with H.LDMatrix.from_scipy(c[form]) as ld:
        assert ld.kind == "sparse" and ld.shape == (c["m"], c["m"]) and ld.nnz == c[form].nnz
        return H.SBayesS(c["ss"], ld, model, Pi, **kw)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name,mname,model,Pi,fold", CASES, ids=["%s-%s" % (x[0], x[1]) for x in CASES])
def test_every_sweep_against_the_sequential_chain(name, mname, model, Pi, fold, form):
    c = case(name)
    ref, moves = reference(name, mname, model, form == "nz")
    r = run(name, form, model, Pi, fold)
    assert r["n_records"] == 3 and r["timing"]["iters_done"] == 3
    _compare(r, ref, 1e-6 if model == "BayesL" else 1e-9)
    np.testing.assert_allclose(r["MCMCsamples"]["Vg"][0], ref["s_Vg"], rtol=1e-6 if model == "BayesL" else 1e-9)
    np.testing.assert_allclose(r["MCMCsamples"]["Ve"][0], ref["s_Ve"], rtol=1e-6 if model == "BayesL" else 1e-9)
    assert np.array_equal(r["g_last"], r["MCMCsamples"]["alpha"][:, -1]) and np.any(r["g_last"] != 0)
    # ---- r_hat = xy - n ldm g, from the device's own g_last ----
    ld, b = c["dense"].astype(np.longdouble), c["ss"][:, 1]
    xy = np.where(np.isnan(b), 0.0, r["n"] * np.diag(c["dense"]) * np.nan_to_num(b)).astype(np.longdouble)
    want = xy - r["n"] * (ld @ r["g_last"].astype(np.longdouble))
    err = float(np.abs(r["r_hat"] - want).max())
    print("%s %s %s: max |r_hat - (xy - n ldm g)| = %.3g, bound %.3g" % (name, mname, form, err, 1e-9 * float(np.abs(xy).max())))
    np.testing.assert_allclose(r["r_hat"], want.astype(np.float64), rtol=0, atol=1e-9 * float(np.abs(xy).max()))
    # ---- the device's count of moves: integers, exactly the trace's ----
    counted = r["timing"]["mean_events"] * r["timing"]["iters_done"]
    print("%s %s %s: moves counted %.17g, the trace's %d" % (name, mname, form, counted, moves))
    assert abs(counted - round(counted)) < 1e-6 and round(counted) == moves   # (mean_events is a sum of integers divided by 3)


def test_two_dense_runs_of_one_call_agree_bit_for_bit():
    _, _, model, Pi, fold = CASES[0]
    a, b = run("rounds", "dense", model, Pi, fold), run("rounds", "dense", model, Pi, fold)
    assert model == "BayesCpi" and same_run(a, b) and np.any(a["MCMCsamples"]["alpha"] != 0)
