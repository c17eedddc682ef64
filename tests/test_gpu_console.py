"""The console lines of a run (src/Bayes.cpp:393-461 and :884-914, src/SBayesD.cpp:190-246 and :514-537): the header block, one progress line per
iteration, and on every progress line of a stored iteration that iteration's Vg, Ve, h2 and pi as MCMCsamples holds them. Both runs take the
progress line from hb_model.hpp (tests/test_model_host.py checks its format alone); this is the line as a run prints it."""
import re

import numpy as np
import pytest

import hibayes_amd as H

pytestmark = pytest.mark.gpu

N, M, MLD = 256, 1024, 256
KW = dict(niter=6, nburn=2, thin=1, outfreq=1, seed=4321)
CASES = [("BayesCpi", [0.95, 0.05], None), ("BayesL", [0.95, 0.05], None), ("BayesR", [0.875, 0.0625, 0.03125, 0.03125], [0, 1e-2, 1e-4, 1e-3])]
BAYES_HEAD = ["Prior parameters:", "    Model fitted at [", "    Number of observations 256", "    Number of covariates 1", "    Number of envir-random effects 0",
              "    Number of markers 1024", "    Total number of iteration 6", "    Total number of burn-in 2", "    Frequency of collecting 1", "    Phenotypic var ",
              "    Genetic var ", "    Inv-Chisq gpar ", "    Residual var ", "    Inv-Chisq epar ", "    Marker var ", "    Inv-Chisq alpar ", "MCMC started: "]
SBAYES_HEAD = ["Prior parameters:", "    Model fitted at [", "    Population size 256", "    Number of markers 256", "    Number of markers used for analysis 256",
               "    Total number of iteration 6", "    Total number of burn-in 2", "    Phenotypic var ", "    Genetic var ", "    Inv-Chisq gpar ", "    Residual var ",
               "    Inv-Chisq epar ", "    Marker var ", "    Inv-Chisq alpar ", "MCMC started: "]


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(12)
    p = rng.uniform(0.1, 0.5, M)
    X = ((rng.random((N, M)) < p).astype(np.int8) + (rng.random((N, M)) < p).astype(np.int8))
    beta = np.zeros(M)
    beta[rng.choice(MLD, 8, replace=False)] = rng.normal(0, 1, 8)
    y = X @ beta + rng.normal(0, 1.0, N)
    Xl = X[:, :MLD].astype(float)
    Xc = Xl - Xl.mean(0)
    xx = (Xc ** 2).sum(0)
    b = (Xc * (y - y.mean())[:, None]).sum(0) / xx
    se = np.sqrt(((y - y.mean()) ** 2).sum() / (N - 2) / xx)
    return dict(y=y, X=np.asfortranarray(X), ld=np.cov(Xl, rowvar=False, ddof=0), ss=np.column_stack([Xl.mean(0) / 2, b, se, np.full(MLD, float(N))]))


def check_lines(lines, head, tail, model, r, n_pi):
    """header, one progress line per iteration with the stored iterations' records at four decimals, the closing block"""
    niter, nburn = KW["niter"], KW["nburn"]
    body = len(head) + 1
    assert len(lines) == body + niter + len(tail), "\n".join(lines)
    for got, want in zip(lines, head):
        assert got.startswith(want) and (got == want or want[-1] in " ["), (got, want)
    assert lines[len(head)] == " Iter  NumNZSnp  pi  %sVg  Ve  h2  Timeleft" % ("Lambda  " if model == "BayesL" else "")
    mc = r["MCMCsamples"]
    assert mc["Vg"].shape == (1, niter - nburn) and np.asarray(mc["pi"]).shape == (n_pi, niter - nburn)
    for it in range(niter):
        tok = lines[body + it].split(" ")
        assert tok[0] == "" and tok[1] == str(it + 1) and re.fullmatch(r"\d+", tok[2]), lines[body + it]
        assert len(tok) == 3 + n_pi + (model == "BayesL") + 4, lines[body + it]
        assert all(re.fullmatch(r"\d+\.\d{4}", t) for t in tok[3:-1]) and re.fullmatch(r"\d\dh\d\dm\d\ds", tok[-1]), lines[body + it]
        if it >= nburn:  # thin = 1: record it - nburn
            k = it - nburn
            assert tok[3:3 + n_pi] == ["%.4f" % v for v in np.asarray(mc["pi"])[:, k]], lines[body + it]  # (the caller's class order)
            assert tok[-4:-1] == ["%.4f" % mc["Vg"][0, k], "%.4f" % mc["Ve"][0, k], "%.4f" % mc["h2"][0, k]], lines[body + it]
    for got, want in zip(lines[body + niter:], tail):
        assert got.startswith(want), (got, want)


@pytest.mark.parametrize("model,Pi,fold", CASES)
def test_bayes_prints_its_header_and_one_progress_line_per_iteration(data, model, Pi, fold):
    lines = []
    r = H.Bayes(data["y"], data["X"], model, Pi, fold=fold, log=lines.append, **KW)
    check_lines(lines, BAYES_HEAD, ["Posterior parameters:", "    Mu ", "    Genetic var ", "    Residual var ", "    Estimated h2 ", "Finished: "], model, r, len(Pi))
    if model == "BayesR":  # an unsorted `fold`: the classes' records differ, so the order shows
        assert len({tuple(row) for row in np.asarray(r["MCMCsamples"]["pi"])}) == 4


def test_sbayesd_prints_the_same_lines_from_the_same_function(data):
    model, Pi, fold = CASES[2]
    lines = []
    r = H.SBayesD(data["ss"], data["ld"], model, Pi, fold=fold, log=lines.append, **KW)
    check_lines(lines, SBAYES_HEAD, ["Posterior parameters:", "    Genetic var ", "    Residual var ", "    Estimated h2 ", "Finished: "], model, r, len(Pi))
