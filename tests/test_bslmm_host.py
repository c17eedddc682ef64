"""BSLMM without a GPU: the numpy restatement (tests/bslmm_restatement.py) pinned to the C oracle, what the order of summation alone does
to a chain, the GRM's integer arithmetic against exact rational values, the C ABI's new entries and the Python refusals."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import hibayes_amd as H
from hibayes_amd import _lib
from oracle import oracle as O

import bslmm_restatement as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(niter=60, nburn=20, thin=2, seed=20251019)
NEW = ["hb_grm_build", "hb_grm_free", "hb_ctx_poly_setup", "hb_ctx_poly_step", "hb_ctx_poly_state", "hb_ctx_poly_debug_get",
       "hb_bayes_run_poly", "hb_run_poly"]


def demo_eigen(M, lambda_):
    raw = B.grm_expression(M)
    G = raw / (np.trace(raw) / raw.shape[0])
    G[np.diag_indices_from(G)] += lambda_
    return np.linalg.eigh(G)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def test_restatement_without_Ki_is_the_oracles_bayescpi(demo):
    got = B.bslmm(demo["y"], demo["M"], [0.95, 0.05], **KW)
    ref = O.bayes(demo["y"], demo["M"], "BayesCpi", [0.95, 0.05], rng=O.RNG_PHILOX, store_alpha=True, **KW)
    assert rel(got["s_alpha"], ref["s_alpha"]) < 1e-6          # smoke()'s criterion
    for k in ("Vg", "Ve", "mu"):
        assert abs(got[k] - ref[k]) <= 1e-6 * abs(ref[k]), k


def test_two_summation_orders_give_one_chain(demo):
    """The three products with K in two orders of summation: the chains' relative spread over 60 iterations stays below 1e-9 at
    lambda = 0.01 (at lambda = 0 the smallest eigenvalue is rounding noise, q = sum Kg^2 / Kval amplifies it, and trajectories are not
    comparable: measured 2e-10 after one block at n = 300). This is what keeps the GPU tests' tolerance — 1000 spreads — meaningful."""
    Kval, K = demo_eigen(demo["M"], 0.01)
    a = B.bslmm(demo["y"], demo["M"], [0.95, 0.05], Kival=Kval, Ki=K, order="blas", **KW)
    b = B.bslmm(demo["y"], demo["M"], [0.95, 0.05], Kival=Kval, Ki=K, order="rev", **KW)
    spread = {"alpha": rel(a["s_alpha"], b["s_alpha"]), "k": rel(a["traj"]["k"], b["traj"]["k"]), "Vb": rel(a["traj"]["vb"], b["traj"]["vb"])}
    print("order-to-order spread:", spread)
    assert max(spread.values()) < 1e-9, spread
    assert np.all(np.isfinite(a["ghat"])) and a["Vb"] > 0 and a["Va"] > 0


@pytest.mark.parametrize("codes", [(0, 3), (-1, 2), (-127, 128)])
def test_grm_expression_against_exact_rationals(codes):
    rng = np.random.default_rng(17)
    M = rng.integers(codes[0], codes[1], size=(17, 203)).astype(np.int8)
    err, bound = B.grm_raw_error(M, B.grm_expression(M))
    assert np.all(err <= bound), float(np.max(err / bound))
    # the bound itself stays inside what DESIGN.md section 15 may claim at most: 8 eps times the sum of the three magnitudes
    S, a, Cc = B.grm_integers(M)
    assert np.all(bound <= 8 * B.EPS * (np.abs(S) + np.abs(a[:, None] + a[None, :]) / 17 + Cc / 17 ** 2))


def test_header_symbols_and_struct_layout():
    hdr = open(os.path.join(ROOT, "include", "hibayes_gpu.h")).read()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, hdr), s + " is not declared in the header"
        assert s in _lib.SYMBOLS, s + " is missing from SYMBOLS"
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sz.c"), os.path.join(d, "sz")
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "hibayes_gpu.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n",'
                             'sizeof(hb_poly_out),offsetof(hb_poly_out,Vb),offsetof(hb_poly_out,Vb_sd),offsetof(hb_poly_out,s_Va),'
                             'offsetof(hb_poly_out,s_Vb),offsetof(hb_poly_out,k_mean),offsetof(hb_poly_out,ghat));return 0;}\n')
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    P = _lib.PolyOut
    assert got == [C.sizeof(P), P.Vb.offset, P.Vb_sd.offset, P.s_Va.offset, P.s_Vb.offset, P.k_mean.offset, P.ghat.offset]
    assert H.lib().hb_abi_version() == 6
    assert "make_grm" in H.__all__


def test_python_refusals_that_need_no_device():
    y, X = np.arange(5.0), np.zeros((5, 3), dtype=np.int8)
    with pytest.raises(H.HibayesError, match="variance-covariance matrix should be in square."):
        H.Bayes(y, X, "BSLMM", [0.95, 0.05], Kival=np.ones(5), Ki=np.ones((5, 4)))
    with pytest.raises(H.HibayesError, match="Number of individuals not equals."):
        H.Bayes(y, X, "BSLMM", [0.95, 0.05], Kival=np.ones(4), Ki=np.eye(4))
    with pytest.raises(H.HibayesError, match="one eigenvalue per individual"):
        H.Bayes(y, X, "BSLMM", [0.95, 0.05], Kival=np.ones(4), Ki=np.eye(5))
    with pytest.raises(NotImplementedError, match="inverse"):
        H.make_grm(X, inverse=True)
    L = H.lib()
    assert L.hb_grm_build(None, 0.0, 0, None, None) == 1 and L.hb_last_error().decode() == "hb_grm_build: null context"
    assert L.hb_ctx_poly_step(None, 1.0, 1.0, 1, 0, 1.0, 0.0) == 1
    assert L.hb_run_poly(None, None) == 1
