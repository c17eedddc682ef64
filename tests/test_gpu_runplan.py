"""From plan to context: a run on a context of its own takes the panel, geometry, regime and layout that hb_runplan.hpp states.

tests/test_host_logic.py checks hb_runplan.hpp's functions against tests/golden/run_plan_table.json without a device. It cannot see
whether hb_ctx_create, hb_run's set-up and step apply the answers. Here a pre-loaded Context is configured BY HAND from the recorded
table, and the run on it must be the run that chose for itself."""
import numpy as np
import pytest

import hibayes_amd as H
from run_plan_record import recorded_run_plan

pytestmark = pytest.mark.gpu

MODEL_INDEX = {"BayesRR": 1, "BayesA": 2, "BayesB": 3, "BayesCpi": 4, "BayesL": 5, "BayesR": 6}
N, M_BIG, M_SMALL = 300, 4608, 300   # nine panels of 512; three panels of 128, the last one ragged
CASES = [
    ("BayesRR", [0.95, 0.05], None),
    ("BayesA", [0.95, 0.05], None),
    ("BayesB", [0.8, 0.2], None),
    ("BayesCpi", [0.95, 0.05], None),
    ("BayesL", [0.95, 0.05], None),
    ("BayesR", [0.95, 0.02, 0.02, 0.01], [0, 1e-4, 1e-3, 1e-2]),
    ("BayesR", [0.9375, 0.03125, 0.015625, 0.0078125, 0.0078125], [0, 1e-5, 1e-4, 1e-3, 1e-2]),   # five classes: no geometry by regime
]


@pytest.fixture(scope="module")
def plan():
    return recorded_run_plan()


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(20261018)
    p = rng.uniform(0.05, 0.5, M_BIG)
    X = np.asfortranarray((rng.random((N, M_BIG)) < p).astype(np.int8) + (rng.random((N, M_BIG)) < p).astype(np.int8))
    X[:, 7::997] = 1   # monomorphic markers: skipped by the sweep
    idx = rng.choice(M_BIG, 40, replace=False)
    xb = X[:, idx].astype(np.float64) @ rng.normal(0, 1, 40)
    return {"X": X, "y": xb * np.sqrt(0.5 / xb.var()) + rng.normal(0, np.sqrt(0.5), N)}


def _same(a, b, what):
    if isinstance(a, dict):
        assert set(a) == set(b), what
        for k in a:
            _same(a[k], b[k], "%s[%s]" % (what, k))
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b)), what


@pytest.mark.parametrize("model,Pi,fold,m", [c + (M_BIG,) for c in CASES] + [c + (M_SMALL,) for c in CASES if MODEL_INDEX[c[0]] in (1, 2, 5)])
def test_a_run_on_its_own_context_is_the_run_on_a_context_set_up_from_the_recorded_plan(plan, data, model, Pi, fold, m):
    """H.Bayes(y, X) creates and configures its context from hb_runplan.hpp. The same call on a pre-loaded Context with the panel, the
    geometry, set_adaptive and the layout that tests/golden/run_plan_table.json records for the case is the same chain: alpha, pip, g, pi,
    every MCMCsamples entry and the state after the last sweep (`last`) bit for bit. The layout is the one the first run reports, so a
    device short of memory changes what is compared, not whether it passes; it must be one the table allows.

    `e` alone is not compared bit for bit: e = y - mu - X alpha, and k_xalpha (hb_ingest.hpp) adds its blocks of 256 columns into a row
    with fp64 atomics in no fixed order, so two runs of ONE configuration differ in e's last bits. With B column blocks two orders of
    summation differ by at most 2 (B - 1) u |x_i| . |alpha| (u = 2^-53), and the subtraction adds one rounding of e: the bound below.
    At m = 300 (two blocks: a sum of two terms has one value) the bound is zero and e is compared bit for bit as well."""
    mi, nf = MODEL_INDEX[model], len(Pi)
    X, y = data["X"][:, :m], data["y"]
    kw = dict(fold=fold, niter=24, nburn=4, thin=2, seed=31337, verbose=False)
    # ---- what the record says this run takes (own context, concurrent kernels, no environment switch) ----
    P = int(plan["panel"]["%d %d 0" % (m, int(mi in (1, 2, 5)))])
    asked, made = (tuple(int(x) for x in s.split()) for s in plan["default"]["%d %d %d 0 2 0 1" % (mi, nf, P)].split(" -> "))
    pipeline, Lv, D, L, _ = made
    regime = plan["regime"]["%d %d %d 1 0 0 %d %d %d %d" % (mi, nf, P, L, pipeline, Lv, D)]
    assert P == (512 if m == M_BIG else 128)

    own = H.Bayes(y, X, model, Pi, **kw)
    bits = own["timing"]["resident_bits"]
    if m == M_BIG:   # (the record's layout stage has this m_pad: 2 bits at most where it says so with memory to spare)
        assert bits in (8, int(plan["layout"]["0 1 0 2 0 %d 0 3 3 %d %d %d 2 %d" % (pipeline, P, mi, nf, m)]))
    else:
        assert bits == 8
    with H.Context(N, m, panel=P, seed=31337) as c:
        assert c.panel == P
        c.upload(X)
        c.set_pipeline(*asked)
        assert c.pipeline() == (pipeline, Lv, D, L)
        c.build_gram()
        if bits == 2:
            c.set_layout(2, keep_int8=False)
        c.set_adaptive(regime != "off")
        pre = H.Bayes(y, None, model, Pi, ctx=c, **kw)
        geo_end = c.pipeline()[1:3]
    # geometry by regime: where the record has it, the run ended in one of its two geometries, else in the one it was given
    w = regime.split()
    assert geo_end in ([(Lv, D)] if regime == "off" else [(int(w[1]), int(w[2])), (int(w[4]), int(w[5]))]), (regime, geo_end)
    assert pre["timing"]["resident_bits"] == bits

    for k in ("alpha", "pip", "g", "pi", "Vg", "Ve", "h2", "mu", "MCMCsamples", "last"):
        _same(own[k], pre[k], k)
    blocks = -(-(-(-m // P) * P) // 256)   # k_xalpha's column blocks over the padded markers
    bound = np.finfo(np.float64).eps * (blocks * (np.abs(X).astype(np.float64) @ np.abs(own["alpha"])) + np.abs(own["e"])) if blocks > 2 else np.zeros(N)
    err = np.abs(own["e"] - pre["e"])
    print("%s m=%d: panel %d, geometry %s, regime '%s', %d bits; max |e - e'| = %.3g (bound %.3g)" % (model, m, P, made[:3], regime, bits, err.max(), bound.max()))
    assert np.all(err <= bound), "e differs by %g, bound %g" % (err.max(), bound[np.argmax(err - bound)])
