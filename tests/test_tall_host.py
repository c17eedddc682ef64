"""What test_gpu_tall.py relies on, without a device: the integer restatement of the fixed-point mat-vec holds its own
properties, and hb_matvecplan.hpp gives the tall columns of that file the tiles it says it tests."""
import os
import random
import subprocess

import numpy as np

from tall_restatement import (CAP_ROWS, HB_ND, Q_HIGH, Q_LOW, digit_planes, digits_of, horner, limbs18, quantise, restate, tall_genotypes,
                              tall_residuals, ulps_off)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_digits_of_the_edge_integers():
    """Worked by hand from hb_store_digits: 0x80 in a byte is digit -128 and a carry into the next plane; -q is not the digits negated."""
    assert digits_of(Q_LOW) == [-128, -128, -128, -128, -128, -128, 64]
    assert digits_of(-Q_LOW) == [-128, -127, -127, -127, -127, -127, -63]
    assert digits_of(Q_HIGH) == [127, 127, 127, 127, 127, 127, 31]
    assert digits_of(2 ** 53) == [0, 0, 0, 0, 0, 0, 32] and digits_of(0) == [0] * HB_ND
    # doubles: the quantiser's own integers at E = 53 — q_low where every row holds it, q_high beside a row at 1.0 = 2^53 2^-53
    assert 2 ** 53 <= Q_LOW < 2 ** 54 and 2 ** 52 <= Q_HIGH < 2 ** 53 and int(float(Q_LOW)) == Q_LOW and int(float(Q_HIGH)) == Q_HIGH


def test_the_digits_recombine_to_q():
    rnd = random.Random(7)
    edge = [0, 1, -1, 127, 128, -128, -129, 255, 256, 2 ** 53, -2 ** 53, 2 ** 54 - 2, -(2 ** 54 - 2), Q_LOW, -Q_LOW, Q_HIGH, -Q_HIGH,
            0x00808080808080, 0x007f7f7f7f7f7f, 0x1fffffffffffff]
    qs = edge + [rnd.randrange(-2 ** 54 + 1, 2 ** 54) for _ in range(2000)] + [rnd.randrange(-2 ** b, 2 ** b) for b in range(1, 54) for _ in range(8)]
    planes = digit_planes(np.array(qs, dtype=np.int64))
    lim = limbs18(np.array(qs, dtype=np.int64))
    for i, q in enumerate(qs):
        d = digits_of(q)
        assert sum(v << (8 * k) for k, v in enumerate(d)) == q
        assert all(-128 <= v <= 127 for v in d[:HB_ND - 1]) and -64 <= d[HB_ND - 1] <= 64, (q, d)
        assert planes[:, i].tolist() == d
        assert int(lim[0, i]) + (int(lim[1, i]) << 18) + (int(lim[2, i]) << 36) == q


def test_the_horner_restatement_against_the_exact_sum():
    """Below 2^61 the partial value before the last step is below 2^53: only that step rounds, and the result is the correctly rounded sum.
    From there on each of the R steps whose exact partial value reaches 2^53 rounds once, by at most half an ulp of a partial value that
    the later steps scale with the sum: within R / 2 ulp."""
    rnd = random.Random(11)
    seen, worst = set(), 0.0
    for _ in range(6000):
        top = rnd.randrange(0, HB_ND)
        acc = [rnd.randrange(-2 ** 38, 2 ** 38) if k <= top else 0 for k in range(HB_ND)]
        acc[top] = rnd.randrange(-2 ** rnd.randrange(1, 39), 2 ** rnd.randrange(1, 39))
        E = rnd.randrange(-60, 120)
        v, exact, R = horner(acc, E)
        assert exact == sum(a << (8 * k) for k, a in enumerate(acc))
        u = ulps_off(v, exact, E)
        if abs(exact) < 2 ** 61:
            assert R <= 1 and v == np.ldexp(float(exact), -E), (acc, E)
        assert u <= R / 2, (acc, u, R)
        seen.add(R)
        worst = max(worst, u / max(R, 1) * 2)
    assert seen == set(range(6)), seen                  # sums up to 2^86: none to five rounding steps
    print("Horner restatement: at most %.3f of R / 2 ulp" % worst)


def test_restate_on_a_small_column_set():
    """restate() end to end where Python integers can check all of it: the planes are the digits, the sums the products, E the exponent."""
    n = 1500
    X, X8 = tall_genotypes(n, 64, 3)
    for name, r in tall_residuals(n, 4).items():
        ref = restate(X8, r)
        E, q = quantise(r)
        assert ref["E"] == E == (0 if not r.any() else 53 - int(np.floor(np.log2(np.abs(r).max())))), name
        qi = [int(v) for v in q]
        for i in (0, 1, n // 3, n - 1):
            assert ref["planes"][:, i].tolist() == digits_of(qi[i]), (name, i)
        for j in range(0, 64, 7):
            col = [int(x) for x in X8[:, j]]
            assert ref["exact"][j] == sum(x * v for x, v in zip(col, qi)), (name, j)
            for k in range(HB_ND):
                assert int(ref["acc"][j, k]) == sum(x * int(d) for x, d in zip(col, ref["planes"][k])), (name, j, k)
    assert (X[:, 1] == 3).all() and not X[:, 2].any() and X[:, 3].sum() == 3 and X[n - 1, 3] == 3
    assert (X8[:, 5] == 127).all() and (X8[:, 6] == -127).all() and (X8[:, 8] == -128).all() and X8[:4, 7].tolist() == [127, -127, 127, -127]


_PLAN_PROGRAM = r"""
#include "hb_matvecplan.hpp"
#include <cstdio>
static void row(const char *what, long long n, const hb_matvec_knobs &k, int layout)
{
    const long long ld = (n + 255) / 256 * 256, ld2 = 128 * ((ld + 511) / 512);
    const hb_matvec_plan p = plan_matvec(hb_matvec_shape{layout, ld, ld2, 64, 0, 0, false, 256}, k);
    printf("%s %lld | %lld %d %d %d %d %d %d\n", what, n, ld, p.family, p.arg[0], p.arg[1], p.nstages, p.NS, p.tiles);
}
int main()
{
    for (long long n : {131072LL, 131073LL, 174001LL, 262145LL, 700001LL}) {
        for (int forced = 0; forced < 2; forced++) {
            hb_matvec_knobs k;
            if (forced) k.dotq_tiles = 1, k.dotq2_tiles = 1, k.dotq2_tiles_set = true;
            const char *f = forced ? "one" : "default";
            char what[64];
            snprintf(what, sizeof what, "%s dotq", f); row(what, n, k, 8);
            k.kind = 0; snprintf(what, sizeof what, "%s dotq2", f); row(what, n, k, 2);
            k.kind = 1; snprintf(what, sizeof what, "%s dotq2r", f); row(what, n, k, 2);
            k.kind = 2; k.q2m_g = 0; snprintf(what, sizeof what, "%s dotq2m-g0", f); row(what, n, k, 2);
            k.q2m_g = 1; snprintf(what, sizeof what, "%s dotq2m-g1", f); row(what, n, k, 2);
        }
    }
}
"""


def test_the_plan_gives_the_tall_columns_the_tiles_the_gpu_file_means(tmp_path):
    """hb_matvecplan.hpp on the CPU (g++, as test_host_logic.py runs it), one panel of 64 columns as hb_ctx_dot launches it, with
    HB_DOTQ_TILES = 1 / HB_DOTQ2_TILES = 1 and with the defaults. Forced to one tile the int8 cap binds at every size of test_gpu_tall.py
    (tiles of 1023 stages = 130 944 rows), the 2-bit floor from ld = 131 328 on; with the defaults neither does (NS = 2 at ld = 131 072),
    which is why that file sets the knobs. Rows of a tile = NS x rows per stage (128, 256, or 512 for k_dotq2m's G = 0, which needs ld to be
    a multiple of 512 and is G = 1 otherwise); k_dotq2r's tiles are its row blocks of 4 096."""
    src, exe = tmp_path / "tallplan.cpp", tmp_path / "tallplan"
    src.write_text(_PLAN_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "hibayes_amd", "csrc"), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        k, v = line.split(" | ")
        got[k] = tuple(int(x) for x in v.split())
    DOTQ2, DOTQ2M, DOTQ2R, DOTQ = 0, 1, 2, 3
    # (ld, family, template arguments, stages of a column, stages per tile, tiles)
    want = {
        "one dotq 131072": (131072, DOTQ, 0, 0, 1024, 1023, 2),            # 1023 stages and 1: a tile of 1024 would hold 2^31 / 128^2 rows
        "one dotq 131073": (131328, DOTQ, 0, 0, 1026, 1023, 2),
        "one dotq 174001": (174080, DOTQ, 0, 0, 1360, 1023, 2),
        "one dotq 262145": (262400, DOTQ, 0, 0, 2050, 1023, 3),
        "one dotq2 131072": (131072, DOTQ2, 1, 256, 512, 512, 1),          # one tile of 131 072 rows
        "one dotq2 131073": (131328, DOTQ2, 1, 256, 513, 257, 2),          # two of 65 792
        "one dotq2 174001": (174080, DOTQ2, 1, 256, 680, 340, 2),          # two of 87 040
        "one dotq2 262145": (262400, DOTQ2, 1, 256, 1025, 342, 3),         # three of 87 552
        "one dotq2 700001": (700160, DOTQ2, 1, 256, 2735, 456, 6),         # six of 116 736
        "one dotq2m-g0 131072": (131072, DOTQ2M, 4, 0, 256, 256, 1),
        "one dotq2m-g0 131073": (131328, DOTQ2M, 4, 1, 513, 257, 2),       # (ld is no multiple of 512: G = 1)
        "one dotq2m-g0 174001": (174080, DOTQ2M, 4, 0, 340, 170, 2),
        "one dotq2m-g0 262145": (262400, DOTQ2M, 4, 1, 1025, 342, 3),
        "one dotq2m-g0 700001": (700160, DOTQ2M, 4, 1, 2735, 456, 6),
        "one dotq2m-g1 131072": (131072, DOTQ2M, 4, 1, 512, 512, 1),
        "one dotq2m-g1 174001": (174080, DOTQ2M, 4, 1, 680, 340, 2),
        "one dotq2r 131072": (131072, DOTQ2R, 0, 0, 32, 16, 128),          # 32 row blocks x 4 groups of 16 columns
        "one dotq2r 131073": (131328, DOTQ2R, 0, 0, 33, 16, 132),
        "one dotq2r 174001": (174080, DOTQ2R, 0, 0, 43, 16, 172),
        "one dotq2r 262145": (262400, DOTQ2R, 0, 0, 65, 16, 260),
        "default dotq 131072": (131072, DOTQ, 0, 0, 1024, 2, 512),         # the defaults: the cap is nowhere near
        "default dotq 262145": (262400, DOTQ, 0, 0, 2050, 3, 684),
    }
    for k, w in want.items():
        assert got[k] == w, (k, got[k], w)
    for k, (ld, family, a0, a1, nst, NS, tiles) in got.items():
        if family == DOTQ:
            assert NS * 128 <= CAP_ROWS and CAP_ROWS * 128 * 128 < 2 ** 31 <= (CAP_ROWS + 128) * 128 * 128, k
        elif family != DOTQ2R:
            rs = 512 if (family == DOTQ2M and a1 in (0, 3)) else 256
            assert NS * rs <= 131072 and -(-131072 // 4) * 96 * 128 < 2 ** 31, k
            if not k.startswith("one"):
                assert NS * rs < 65536, k              # the defaults never come near the floor at these sizes
    # the bound the 2-bit comments state: the scale-32 accumulator sees a quarter of a tile's rows
    assert 4 * 2 ** 31 // (96 * 128) == 699050 and 174762 * 96 * 128 < 2 ** 31 <= 174763 * 96 * 128
    # ... and the test's tallest column passes it in one tile, so without the floor the all-3 column overflows: 700 416 rows, 175 001 threes
    assert -(-700001 // 4) * 96 * 128 >= 2 ** 31


def test_the_extreme_fixtures_are_extreme():
    """The sums test_gpu_tall.py means to be extreme, from the restatement alone: +-127 against planes of -128 over 131 072 rows is
    2 130 706 432 = 0.992 of 2^31, -128 is 2^31 itself, and the tallest tile the plan allows (1023 stages) keeps -128 at 0.999 of it."""
    n = 131072
    X = np.zeros((n, 64), dtype=np.int8, order="F")
    X[:, 0], X[:, 1], X[:, 2] = 127, -127, -128
    ref = restate(X, tall_residuals(n, 1)["every row at q_low"])
    assert ref["E"] == 53 and (ref["planes"][:6] == -128).all() and (ref["planes"][6] == 64).all()
    assert ref["acc"][0, :6].tolist() == [-2130706432] * 6 and ref["acc"][1, :6].tolist() == [2130706432] * 6
    assert ref["acc"][2, :6].tolist() == [2 ** 31] * 6
    assert CAP_ROWS * 128 * 128 == 2145386496 < 2 ** 31
    big = restate(X, tall_residuals(n, 1)["one row at 1, the others at q_high"])
    assert big["acc"][0, 0] == 127 * 127 * (n - 1) and big["R"].max() >= 2
