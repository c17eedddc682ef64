"""hb_model.hpp — the model layer shared by hb_run.hip and hb_sbayes.hip — is plain C++: compiled here with g++ (no HIP include path) into a
driver that reads one case per line, and checked against values this file computes itself from the reference's formulas
(src/Bayes.cpp:92-117, :288-296, :603, :666-669, :710-716, :738-741, :803-814, :1030; src/stats.cpp:69-76; src/SBayesD.cpp:33-34)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hibayes_amd", "csrc")

_DRIVER = r"""
#include "hb_model.hpp"
#include <cstdio>
#include <iostream>
#include <sstream>

struct fake_stream { // records every call, returns the scripted values in turn
    std::vector<double> script;
    size_t at = 0;
    double next() { return at < script.size() ? script[at++] : (at++, 1.0); }
    double chisq(double df) { printf("chisq %a;", df); return next(); }
    double gamma(double shape, double scale) { printf("gamma %a %a;", shape, scale); return next(); }
};

static std::vector<double> vec(std::istringstream &in)
{
    int k;
    in >> k;
    std::vector<double> v(k < 0 ? 0 : k);
    for (double &x : v) { std::string t; in >> t; x = strtod(t.c_str(), nullptr); }
    return v;
}
static double num(std::istringstream &in) { std::string t; in >> t; return strtod(t.c_str(), nullptr); }
static void put(const char *name, const std::vector<double> &v) { printf("|%s", name); for (double x : v) printf(" %a", x); }

int main()
{
    std::string l;
    while (std::getline(std::cin, l)) {
        std::istringstream in(l);
        std::string what;
        in >> what;
        if (what == "index") {
            std::string model;
            in >> model;
            printf("%d\n", hb_model_index(model));
        } else if (what == "mix") { // model index null_pi n_pi_arg Pi.. has_fold n_fold_arg fold..
            std::string model, err;
            int index, null_pi, n_pi, has_fold, n_fold;
            in >> model >> index >> null_pi >> n_pi;
            std::vector<double> pin = vec(in);
            in >> has_fold >> n_fold;
            std::vector<double> fin = vec(in);
            std::vector<double> Pi, fold;
            std::vector<int> cls_of;
            bool fixpi = false, always_in = false;
            int stage = 1, rc = hb_mixture_take(model, null_pi ? nullptr : pin.data(), n_pi, has_fold ? fin.data() : nullptr, n_fold, Pi, fold, err);
            if (!rc) { stage = 2; rc = hb_mixture_always_in(model, index, Pi, fixpi, always_in, err); }
            if (!rc) { stage = 3; rc = hb_mixture_order(index, Pi, fold, cls_of, err); }
            printf("%d|%d|%s|%d %d|cls", rc, rc ? stage : 0, err.c_str(), (int)fixpi, (int)always_in);
            for (int c : cls_of) printf(" %d", c);
            put("Pi", Pi);
            put("fold", fold);
            printf("\n");
        } else if (what == "draw") { // model n_fold fixpi dfvara s2varg shape0 rate0 fold.. sum_g2 sum_vargL counts.. n_total nvar0 varg lambda lambda2 NnzSnp Pi.. script..
            int model, n_fold, fixpi;
            in >> model >> n_fold >> fixpi;
            const double dfvara = num(in), s2varg = num(in), shape0 = num(in), rate0 = num(in);
            std::vector<double> fold = vec(in);
            const double sum_g2 = num(in), sum_vargL = num(in);
            std::vector<double> counts = vec(in);
            const double n_total = num(in), nvar0 = num(in);
            double varg = num(in), lambda = num(in), lambda2 = num(in);
            long long NnzSnp = (long long)num(in);
            std::vector<double> Pi = vec(in), vara_fold(n_fold, -1.0), fsn(n_fold, -1.0);
            fake_stream hs;
            hs.script = vec(in);
            hb_draw_hyper(hs, hb_hyper_prior{model, n_fold, fixpi != 0, dfvara, s2varg, shape0, rate0, fold.data()},
                          hb_hyper_sums{sum_g2, sum_vargL, counts.data(), n_total, nvar0},
                          hb_hyper_state{varg, lambda, lambda2, NnzSnp, Pi.data(), vara_fold.data(), fsn.data()});
            printf("|state %a %a %a %lld", varg, lambda, lambda2, NnzSnp);
            put("Pi", Pi);
            put("vara_fold", vara_fold);
            put("fsn", fsn);
            printf("\n");
        } else if (what == "pip") {
            const double count = num(in);
            int nzct;
            in >> nzct;
            printf("%a\n", hb_pip(count, nzct));
        } else if (what == "n") { // lds m, then the 4 x lds table row by row
            int lds, m;
            in >> lds >> m;
            std::vector<double> ss = vec(in);
            printf("%d\n", hb_sumstat_n(ss.data(), lds, m));
        } else if (what == "prior") { // has_vg has_ve has_dfve has_s2vg has_s2ve vg ve dfve s2vg s2ve dfvara vary h2 nr Pi0 sumvx fold..
            hb_prior_args p{};
            in >> p.has_vg >> p.has_ve >> p.has_dfve >> p.has_s2vg >> p.has_s2ve;
            p.vg = num(in), p.ve = num(in), p.dfve = num(in), p.s2vg = num(in), p.s2ve = num(in);
            p.dfvara = num(in), p.vary = num(in), p.h2 = num(in);
            in >> p.nr;
            p.Pi0 = num(in), p.sumvx = num(in);
            std::vector<double> fold = vec(in), vf(fold.size(), -1.0);
            const hb_priors d = hb_prior_defaults(p, fold.data(), (int)fold.size(), vf.data());
            put("d", {d.vara, d.vare, d.dfvare, d.s2vara, d.varg, d.s2varg, d.s2vare, d.lambda2, d.lambda, d.shape0, d.rate0});
            put("vara_fold", vf);
            printf("\n");
        } else if (what == "sweep") { // model Pi.. fold.. vara_fold.. vare varg s2varg_df dfvara lambda lambda2 iter nburn thin always_in
            int model, iter, nburn, thin, always_in;
            in >> model;
            std::vector<double> Pi = vec(in), fold = vec(in), vf = vec(in);
            const double vare = num(in), varg = num(in), s2df = num(in), dfvara = num(in), lambda = num(in), lambda2 = num(in);
            in >> iter >> nburn >> thin >> always_in;
            const hb_sweep_in s = hb_sweep_params(model, (int)Pi.size(), Pi.data(), fold.data(), vf.data(), vare, varg, s2df, dfvara, lambda, lambda2, iter,
                                                  nburn, thin, always_in != 0);
            printf("%d %d %lld %d %d", s.model_index, s.n_fold, (long long)s.iter, s.count_pip, s.store);
            put("scalars", {s.vare, s.varg, s.s2varg_df, s.dfvara, s.lambda, s.lambda2});
            put("logpi", std::vector<double>(s.logpi, s.logpi + HB_MAX_FOLD));
            put("fold", std::vector<double>(s.fold, s.fold + HB_MAX_FOLD));
            put("vara_fold", std::vector<double>(s.vara_fold, s.vara_fold + HB_MAX_FOLD));
            printf("\n");
        } else if (what == "line") { // iter niter NnzSnp Pi.. cls_of.. extras ('_' for a blank, '-' for none) vara vare vt seconds
            int iter, niter;
            long long nnz;
            in >> iter >> niter >> nnz;
            std::vector<double> Pi = vec(in), cl = vec(in);
            std::vector<int> cls_of(cl.begin(), cl.end());
            std::string extras;
            in >> extras;
            if (extras == "-") extras.clear();
            std::replace(extras.begin(), extras.end(), '_', ' ');
            const double vara = num(in), vare = num(in), vt = num(in), seconds = num(in);
            printf("[%s]\n", hb_progress_line(iter, niter, nnz, Pi.data(), cls_of.data(), (int)Pi.size(), extras.c_str(), vara, vare, vt, seconds).c_str());
        }
    }
    return 0;
}
"""


def _h(x):
    return float(x).hex()


def _v(xs):
    return "%d %s" % (len(xs), " ".join(_h(x) for x in xs))


def arma_sum(v):
    """arma::sum: two interleaved accumulators (restated here, not taken from the header)"""
    a1 = a2 = 0.0
    j = 1
    while j < len(v):
        a1 += v[j - 1]
        a2 += v[j]
        j += 2
    if j - 1 < len(v):
        a1 += v[j - 1]
    return a1 + a2


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("model_host")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(_DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)])

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


def test_the_header_compiles_alone_with_werror_and_no_hip(tmp_path):
    src = tmp_path / "only.cpp"
    src.write_text('#include "hb_model.hpp"\nint main() { return hb_model_index("BayesR") == 6 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(tmp_path / "only")])
    subprocess.check_call([str(tmp_path / "only")])
    text = open(os.path.join(CSRC, "hb_model.hpp")).read()
    assert "#include <hip" not in text and "hb_internal.hpp" not in text


INDEX = {"BayesRR": 1, "BayesA": 2, "BayesB": 3, "BayesBpi": 3, "BayesC": 4, "BayesCpi": 4, "BayesL": 5, "BayesR": 6, "BSLMM": 6, "anything": 6}


def test_model_names_map_to_the_reference_indices(driver):
    names = sorted(INDEX)
    assert [int(x) for x in driver(["index " + n for n in names])] == [INDEX[n] for n in names]


def _mix(model, Pi, fold=None, index=None, null_pi=False):
    return "mix %s %d %d %d %s %d %d %s" % (model, INDEX[model] if index is None else index, int(null_pi), len(Pi), _v(Pi),
                                           int(fold is not None), len(fold or []), _v(fold or []))


def _parse_mix(line):
    rc, stage, text, flags, cls, pi, fold = line.split("|")
    fl = [float.fromhex(x) for x in fold.split()[1:]]
    return dict(status=int(rc), stage=int(stage), text=text, fixpi=flags.split()[0] == "1", always_in=flags.split()[1] == "1",
                cls_of=[int(x) for x in cls.split()[1:]], Pi=[float.fromhex(x) for x in pi.split()[1:]], fold=fl)


L2 = "length of Pi should be 2, the first value is the proportion of non-effect markers."
LPF = "length of Pi and fold not equals."


def test_mixture_arguments_accepted(driver):
    P2 = [0.95, 0.05]
    ok = [  # case, fixpi, always_in, cls_of, Pi, fold
        (_mix("BayesRR", P2), True, True, [0, 1], [0.0, 1.0], [0.0, 0.0]),
        (_mix("BayesA", P2), True, True, [0, 1], [0.0, 1.0], [0.0, 0.0]),
        (_mix("BayesL", P2), True, True, [0, 1], [0.0, 1.0], [0.0, 0.0]),
        (_mix("BayesB", P2), True, False, [0, 1], P2, [0.0, 0.0]),
        (_mix("BayesC", P2), True, False, [0, 1], P2, [0.0, 0.0]),
        (_mix("BayesBpi", P2), False, False, [0, 1], P2, [0.0, 0.0]),
        (_mix("BayesCpi", P2), False, False, [0, 1], P2, [0.0, 0.0]),
        (_mix("BSLMM", P2, index=4), False, False, [0, 1], P2, [0.0, 0.0]),  # hb_run.hip's mapping of that name
        (_mix("BayesCpi", P2, fold=[0.0, 1.0]), False, False, [0, 1], P2, [0.0, 1.0]),
        # an always-in model takes more than two classes (the length rule is the point-mass models'): the first two become {0, 1}
        (_mix("BayesRR", [0.5, 0.25, 0.25], fold=[0.0, 1.0, 2.0]), True, True, [0, 1, 2], [0.0, 1.0, 0.25], [0.0, 1.0, 2.0]),
        # BayesR, fold sorted already / unsorted: classes 1.. come out by increasing fold, cls_of maps them back
        (_mix("BayesR", [0.5, 0.25, 0.125, 0.125], fold=[0.0, 1e-4, 1e-3, 1e-2]), False, False, [0, 1, 2, 3], [0.5, 0.25, 0.125, 0.125], [0.0, 1e-4, 1e-3, 1e-2]),
        (_mix("BayesR", [0.5, 0.25, 0.125, 0.125], fold=[0.0, 1e-2, 1e-4, 1e-3]), False, False, [0, 2, 3, 1], [0.5, 0.125, 0.125, 0.25], [0.0, 1e-4, 1e-3, 1e-2]),
        # class 0 is the null class whatever its fold: it is not sorted with the others
        (_mix("BayesR", [0.5, 0.25, 0.25], fold=[5.0, 2.0, 1.0]), False, False, [0, 2, 1], [0.5, 0.25, 0.25], [5.0, 1.0, 2.0]),
        (_mix("BayesR", [0.5, 0.5], fold=[0.0, 1.0]), False, False, [0, 1], [0.5, 0.5], [0.0, 1.0]),
    ]
    for line, (case, fixpi, always_in, cls_of, Pi, fold) in zip(driver([c[0] for c in ok]), ok):
        r = _parse_mix(line)
        assert (r["status"], r["stage"], r["text"]) == (0, 0, ""), case
        assert (r["fixpi"], r["always_in"], r["cls_of"], r["Pi"], r["fold"]) == (fixpi, always_in, cls_of, Pi, fold), case


def test_mixture_arguments_refused_with_the_references_texts(driver):
    refused = [  # case, status, the function that refuses (1: Pi / fold, 2: always-in, 3: BayesR order), text
        (_mix("BayesCpi", [0.95]), 1, 1, "Pi should be a vector."),
        (_mix("BayesCpi", [0.95, 0.05], null_pi=True), 1, 1, "Pi should be a vector."),
        (_mix("BayesR", [0.2] + [0.1] * 8, fold=[float(k) for k in range(9)]), 4, 1, "more mixture classes than HB_MAX_FOLD"),
        (_mix("BayesCpi", [0.5, 0.6]), 1, 1, "sum of Pi should be 1."),
        (_mix("BayesCpi", [1.0, 0.0]), 1, 1, "all markers have no effect size."),
        (_mix("BayesRR", [1.0, 0.0]), 1, 1, "all markers have no effect size."),  # (before the always-in models overwrite Pi)
        (_mix("BayesCpi", [1.5, -0.5]), 1, 1, "elements of Pi should be at the range of [0, 1]"),
        (_mix("BayesR", [0.5, 0.25, 0.25]), 1, 1, "'fold' should be provided for BayesR model."),
        (_mix("BayesR", [0.5, 0.25, 0.25], fold=[0.0, 1e-3]), 1, 1, LPF),
        (_mix("BayesCpi", [0.5, 0.5], fold=[0.0, 1.0, 2.0]), 1, 1, LPF),
        (_mix("BayesCpi", [0.5, 0.25, 0.25]), 1, 1, LPF),  # without fold a model other than BayesR has two zeros for it
        (_mix("BayesRR", [0.5, 0.25, 0.25]), 1, 1, LPF),
        (_mix("BayesCpi", [0.5, 0.25, 0.25], fold=[0.0, 1.0, 2.0]), 1, 2, L2),
        (_mix("BayesB", [0.5, 0.25, 0.25], fold=[0.0, 1.0, 2.0]), 1, 2, L2),
        (_mix("BSLMM", [0.5, 0.25, 0.25], fold=[0.0, 1.0, 2.0], index=4), 1, 2, L2),
        # the summary-level route gives that name BayesR's index and still holds it to two classes
        (_mix("BSLMM", [0.5, 0.25, 0.25], fold=[0.0, 1.0, 2.0]), 1, 2, L2),
        (_mix("BayesR", [0.5, 0.25, 0.25], fold=[0.0, 1e-2, 1e-2]), 4, 3, "BayesR on the GPU path needs distinct 'fold' values for the non-null classes"),
        (_mix("BayesR", [0.5, 0.125, 0.125, 0.25], fold=[0.0, 1e-2, 1e-4, 1e-2]), 4, 3, "BayesR on the GPU path needs distinct 'fold' values for the non-null classes"),
        (_mix("BayesR", [0.5, 0.25, 0.25], fold=[0.0, 1e-2, float("nan")]), 4, 3, "BayesR on the GPU path needs distinct 'fold' values for the non-null classes"),
    ]
    for line, (case, status, stage, text) in zip(driver([c[0] for c in refused]), refused):
        r = _parse_mix(line)
        assert (r["status"], r["stage"], r["text"]) == (status, stage, text), case


# ---- hb_draw_hyper ----
DF, S2, SHAPE0, RATE0 = 4.5, 0.0123, 1.1, 3.7e-4
SUM_G2, SUM_VARGL = 0.8125, 41.3
VARG0, LAM0, LAM20 = 0.0021, 7.5, 56.25


def _draw(model, n_fold, fixpi, fold, counts, n_total, nvar0, Pi, script, nnz0=-7):
    line = "draw %d %d %d %s %s %s %s %s %s %s %s %s %s %s %s %s %d %s %s" % (
        model, n_fold, int(fixpi), _h(DF), _h(S2), _h(SHAPE0), _h(RATE0), _v(fold), _h(SUM_G2), _h(SUM_VARGL), _v(counts), _h(n_total), _h(nvar0),
        _h(VARG0), _h(LAM0), _h(LAM20), nnz0, _v(Pi), _v(script))
    return line


def _parse_draw(line):
    calls, state, pi, vf, fsn = line.split("|")
    cl = []
    for c in calls.split(";"):
        if c:
            t = c.split()
            cl.append((t[0],) + tuple(float.fromhex(x) for x in t[1:]))
    s = state.split()
    f = lambda part: [float.fromhex(x) for x in part.split()[1:]]
    return dict(calls=cl, varg=float.fromhex(s[1]), lam=float.fromhex(s[2]), lam2=float.fromhex(s[3]), nnz=int(s[4]), Pi=f(pi), vara_fold=f(vf), fsn=f(fsn))


def _dirichlet(xn):
    sx = arma_sum(xn)
    return [x / sx for x in xn]


UNTOUCHED = -1.0  # the driver pre-fills vara_fold and fold_snp_num with it


def test_draws_of_the_always_in_models(driver):
    P = [0.0, 1.0]
    # n_total = 1030, nvar0 = 10 straddle 1024: (shape0 + 1030) - 10 and shape0 + 1020 differ in the last bit, and the reference's
    # expression (src/Bayes.cpp:738 `shape0 + m - nvar0`) is the first
    assert (SHAPE0 + 1030.0) - 10.0 != SHAPE0 + 1020.0
    lines = [_draw(1, 2, True, [0.0, 0.0], [0.0, 0.0], 1000.0, 0.0, P, [2.5]),
             _draw(1, 2, True, [0.0, 0.0], [0.0, 0.0], 1030.0, 10.0, P, [2.5]),
             _draw(2, 2, True, [0.0, 0.0], [0.0, 0.0], 1000.0, 3.0, P, [2.5]),
             _draw(5, 2, True, [0.0, 0.0], [0.0, 0.0], 1000.0, 0.0, P, [49.0]),
             _draw(5, 2, True, [0.0, 0.0], [0.0, 0.0], 1030.0, 10.0, P, [49.0])]
    r = [_parse_draw(x) for x in driver(lines)]
    for k, (nt, nv) in ((0, (1000.0, 0.0)), (1, (1030.0, 10.0))):  # :603, one chisq(dfvara + n_used)
        assert r[k]["calls"] == [("chisq", DF + nt - nv)]
        assert r[k]["varg"] == (SUM_G2 + S2 * DF) / 2.5
        assert (r[k]["lam"], r[k]["lam2"], r[k]["nnz"], r[k]["Pi"]) == (LAM0, LAM20, -7, P)
    assert r[0]["calls"] == [("chisq", DF + 1000.0)]
    assert r[2]["calls"] == [] and (r[2]["varg"], r[2]["lam2"], r[2]["nnz"], r[2]["Pi"]) == (VARG0, LAM20, -7, P)  # BayesA: nothing drawn here
    for k, (nt, nv) in ((3, (1000.0, 0.0)), (4, (1030.0, 10.0))):  # :738-741
        assert r[k]["calls"] == [("gamma", SHAPE0 + nt - nv, 1 / (RATE0 + SUM_VARGL / 2))]
        assert (r[k]["lam2"], r[k]["lam"], r[k]["varg"]) == (49.0, 7.0, VARG0)
    assert r[3]["calls"][0][1] == SHAPE0 + 1000.0
    for x in r:
        assert x["vara_fold"] == [UNTOUCHED] * 2 and x["fsn"] == [UNTOUCHED] * 2


@pytest.mark.parametrize("fixpi", [True, False])
def test_draws_of_the_two_class_point_mass_models(driver, fixpi):
    P = [0.95, 0.05]
    counts = [0.0, 37.0]  # only class 1's count is read (:666, :710); class 0 is what is left of the sampled markers
    lines = [_draw(3, 2, fixpi, [0.0, 0.0], counts, 1000.0, 4.0, P, [1.25, 0.75]),
             _draw(4, 2, fixpi, [0.0, 0.0], counts, 1000.0, 4.0, P, [3.5, 1.25, 0.75])]
    b, c = [_parse_draw(x) for x in driver(lines)]
    pi_calls = [("gamma", 959.0 + 1, 1.0), ("gamma", 37.0 + 1, 1.0)]
    newpi = _dirichlet([1.25, 0.75])
    assert b["calls"] == ([] if fixpi else pi_calls)  # BayesB draws no varg
    assert b["varg"] == VARG0
    assert c["calls"] == [("chisq", DF + 37.0)] + ([] if fixpi else pi_calls)  # :713, then :716
    assert c["varg"] == (SUM_G2 + S2 * DF) / 3.5
    for x in (b, c):
        assert x["fsn"] == [959.0, 37.0] and x["nnz"] == 37
        assert x["Pi"] == (P if fixpi else newpi)
        assert x["vara_fold"] == [UNTOUCHED] * 2 and (x["lam"], x["lam2"]) == (LAM0, LAM20)


@pytest.mark.parametrize("fixpi", [True, False])
@pytest.mark.parametrize("n_fold", [4, 5])
def test_draws_of_bayesr(driver, fixpi, n_fold):
    fold = [0.0, 1e-4, 1e-3, 1e-2, 1e-1][:n_fold]
    counts = [900.0, 50.0, 30.0, 15.0, 5.0][:n_fold]
    P = [0.5, 0.25, 0.125, 0.0625, 0.0625][:n_fold]
    P[-1] = 1.0 - sum(P[:-1])
    xn = [0.1, 0.7, 1e-17, 0.3, 0.2][:n_fold]
    if n_fold == 5:  # an odd class count on which the interleaved sum is not the sequential one: the order shows
        assert arma_sum(xn) != sum(xn)
    r = _parse_draw(driver([_draw(6, n_fold, fixpi, fold, counts, 1000.0, 0.0, P, [3.5] + xn)])[0])
    nnz = sum(counts[1:])
    assert r["calls"] == [("chisq", DF + nnz)] + ([] if fixpi else [("gamma", c + 1, 1.0) for c in counts])  # :806, then :814 per class in order
    varg = (SUM_G2 + S2 * DF) / 3.5
    assert r["varg"] == varg and r["nnz"] == int(nnz) and r["fsn"] == counts
    assert r["vara_fold"] == [varg * f for f in fold]
    assert r["Pi"] == (P if fixpi else _dirichlet(xn))
    assert (r["lam"], r["lam2"]) == (LAM0, LAM20)


def test_pip_is_never_exactly_one(driver):
    nzct = 40
    out = [float.fromhex(x) for x in driver(["pip %s %d" % (_h(c), nzct) for c in (0.0, nzct - 1.0, float(nzct))])]
    assert out == [0.0, (nzct - 1.0) / nzct, (nzct - 1) / float(nzct)]
    assert out[2] < 1.0


def test_population_size_is_the_truncated_mean_of_the_finite_n(driver):
    nan, inf = float("nan"), float("inf")

    def case(N, lds=None):
        m = len(N)
        lds = lds or m
        rows = [[float(k) for k in range(lds)], [0.5] * lds, [0.25] * lds, list(N) + [1e9] * (lds - m)]  # (beyond m: never read)
        return "n %d %d %s" % (lds, m, _v([x for row in rows for x in row]))
    got = [int(x) for x in driver([case([100.0, 101.0, 103.0]), case([100.0, nan, 103.0, inf, -inf]), case([nan, nan, inf]), case([250.5, 250.5], lds=5)])]
    assert got == [int((100.0 + 101.0 + 103.0) / 3), int((100.0 + 103.0) / 2), 0, 250]


def _f(part):
    """the doubles of one '|name x x ..' part of a driver line, from their hex"""
    return [float.fromhex(x) for x in part.split()[1:]]


# ---- prior defaults, src/Bayes.cpp:327-374 / src/SBayesD.cpp:117-170 ----
def _priors(has, val, dfvara, vary, h2, nr, pi0, sumvx, fold):
    """the reference's expressions, operand for operand (restated here, not taken from the header)"""
    import math
    vara = val["vg"] if has["vg"] else ((dfvara - 2) / dfvara) * vary * h2
    vare = val["ve"] if has["ve"] else vary * (1 - h2) / (nr + 1)
    dfvare = val["dfve"] if has["dfve"] else -2.0
    s2vara = val["s2vg"] if has["s2vg"] else vara * (dfvara - 2) / dfvara
    varg = vara / ((1 - pi0) * sumvx)
    s2varg = s2vara / ((1 - pi0) * sumvx)
    s2vare = val["s2ve"] if has["s2ve"] else 0.0
    R2 = (dfvara - 2) / dfvara
    lambda2 = 2 * (1 - R2) / (R2) * sumvx
    shape0 = 1.1
    return [vara, vare, dfvare, s2vara, varg, s2varg, s2vare, lambda2, math.sqrt(lambda2), shape0, (shape0 - 1) / lambda2], [(vara / ((1 - pi0) * sumvx)) * f for f in fold]


def test_prior_defaults_are_the_references_expressions(driver):
    import itertools
    import math
    names = ("vg", "ve", "dfve", "s2vg", "s2ve")
    val = dict(vg=3.7, ve=0.9, dfve=5.5, s2vg=0.0123, s2ve=0.77)
    dfvara, vary, h2, pi0, sumvx = 4.5, 215.2144812894398, 0.5, 0.95, 321.987654321
    fold = [0.0, 1e-4, 1e-3, 1e-2]
    cases = [(dict(zip(names, bits)), nr) for bits in itertools.product((0, 1), repeat=5) for nr in (0, 2)]
    lines = ["prior %s %s %s %s %s %d %s %s %s" % (" ".join(str(has[k]) for k in names), " ".join(_h(val[k]) for k in names), _h(dfvara), _h(vary), _h(h2),
                                                    nr, _h(pi0), _h(sumvx), _v(fold)) for has, nr in cases]
    for line, (has, nr) in zip(driver(lines), cases):
        _, d, vf = line.split("|")
        want_d, want_vf = _priors(has, val, dfvara, vary, h2, nr, pi0, sumvx, fold)
        assert _f(d) == want_d, (has, nr)
        assert _f(vf) == want_vf, (has, nr)
    # the random effects share the residual's half of var(y): with two of them the default is a third of it, not all
    assert _priors(dict.fromkeys(names, 0), val, dfvara, vary, h2, 2, pi0, sumvx, fold)[0][1] == vary * 0.5 / 3 != vary * 0.5


def test_sweep_parameters_are_the_chains_state_field_by_field(driver):
    import math
    Pi, fold, vf = [0.5, 0.25, 0.125, 0.125], [0.0, 1e-4, 1e-3, 1e-2], [0.0, 2.1e-7, 2.1e-6, 2.1e-5]
    vare, varg, s2df, dfvara, lam, lam2 = 107.6, 0.0021, 0.0123 * 4.5, 4.5, 7.5, 56.25
    nburn = 10

    def case(it, thin=3, always_in=0):
        return "sweep 6 %s %s %s %s %s %s %s %s %s %d %d %d %d" % (_v(Pi), _v(fold), _v(vf), _h(vare), _h(varg), _h(s2df), _h(dfvara), _h(lam), _h(lam2), it, nburn,
                                                                  thin, always_in)
    its = [nburn - 1, nburn, nburn + 1, nburn + 2, nburn + 3, nburn + 5]
    out = driver([case(it) for it in its] + [case(nburn + 2, thin=0), case(nburn + 2, always_in=1), case(nburn + 2, thin=1), case(nburn - 1, thin=1)])
    pad = lambda xs: list(xs) + [0.0] * (8 - len(xs))
    for line, it in zip(out, its):
        head, sc, lp, fo, vfo = line.split("|")
        assert head.split() == ["6", "4", str(it), str(int(it >= nburn)), str(int(it >= nburn and (it + 1 - nburn) % 3 == 0))], it
        assert _f(sc) == [vare, varg, s2df, dfvara, lam, lam2]
        assert _f(lp) == pad([math.log(p) for p in Pi]) and _f(fo) == pad(fold) and _f(vfo) == pad(vf)
    assert [line.split("|")[0].split()[3:] for line in out[:6]] == [["0", "0"], ["1", "0"], ["1", "0"], ["1", "1"], ["1", "0"], ["1", "1"]]
    # never a record (the summary level), every marker always in (no PIP counts), every iteration after the burn-in, none before
    assert [line.split("|")[0].split()[3:] for line in out[6:]] == [["1", "0"], ["0", "1"], ["1", "1"], ["0", "0"]]


def test_progress_lines_are_the_references_format(driver):
    def case(it, niter, nnz, Pi, cls_of, extras, vara, vare, vt, seconds):
        return "line %d %d %d %s %s %s %s %s %s %s" % (it, niter, nnz, _v(Pi), _v(cls_of), extras.replace(" ", "_") or "-", _h(vara), _h(vare), _h(vt), _h(seconds))
    out = driver([
        case(4, 100, 37, [0.95, 0.05], [0, 1], "", 1.23456, 2.5, 1.23456 + 2.5, 2.0),                                    # BayesCpi
        case(0, 6, 512, [0.5, 0.125, 0.0625, 0.3125], [0, 2, 3, 1], "", 10.0, 30.0, 40.0, 0.25),                         # BayesR, fold = [0, 1e-2, 1e-4, 1e-3]
        case(11, 12, 1024, [0.0, 1.0], [0, 1], "7.5000 ", 0.5, 1.5, 2.5, 600.0),                                         # BayesL; vt with a random effect's variance
        case(9, 1000, 3, [0.9, 0.1], [0, 1], "0.1000 0.2000 0.3000 ", 2.0, 2.0, 4.0, 100.0),                             # extras, 9910 s left
    ])
    assert out == ["[ 5 37 0.9500 0.0500 1.2346 2.5000 0.3306 00h00m38s]",
                   "[ 1 512 0.5000 0.3125 0.1250 0.0625 10.0000 30.0000 0.2500 00h00m01s]",
                   "[ 12 1024 0.0000 1.0000 7.5000 0.5000 1.5000 0.2000 00h00m50s]",
                   "[ 10 3 0.9000 0.1000 0.1000 0.2000 0.3000 2.0000 2.0000 0.5000 02h45m10s]"]
