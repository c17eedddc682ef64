"""The fixed-point mat-vec restated with integers, for columns as tall as its int32 accumulators reach (used by
test_tall_host.py without a device and by test_gpu_tall.py against one).

The device computes d_j = x_j . r as sum_k 256^k (x_j . D_k) 2^-E with D_k the balanced base-256 digit planes of q = rint(r 2^E),
E = 53 - ilogb(max |r|) (hb_fix_exp, hb_store_digits: hb_update.hpp), every x_j . D_k an int32 sum per tile and an int64 sum per column,
and hbq_finalize (hb_matvec.hpp) a Horner recurrence a = fma(a, 256, acc_k) over the seven sums, scaled back by ldexp. Nothing here
multiplies on the kernel's plan: the planes come from integer arithmetic on q, the sums from float64 BLAS on operands whose every partial
sum is an integer below 2^53 (asserted), the recurrence from Python integers (int -> float is correctly rounded, which is the fma).
The exact product it is compared with comes from another split of q (three limbs of 18 bits), not from the planes."""
import math

import numpy as np

HB_ND = 7
# doubles: the quantiser's own integers for r = q 2^-53 at E = 53 (q_low in [2^53, 2^54) where every row holds it, q_high beside a row at 1.0)
Q_LOW = 0x3f7f7f7f7f7f80      # balanced digits (-128, -128, -128, -128, -128, -128, 64)
Q_HIGH = 0x1f7f7f7f7f7f7f     # digits (127, 127, 127, 127, 127, 127, 31): the largest digit in planes 0..5, no carry
CAP_ROWS = 1023 * 128          # rows of the tallest k_dotq tile (plan_matvec): 1023 * 128 * 128 * 128 < 2^31


def digits_of(q):
    """Balanced base-256 digits of the Python integer q as hb_store_digits splits it: planes 0..5 in [-128, 127], lowest first, plane 6
    the remainder."""
    d = []
    for _ in range(HB_ND - 1):
        lo = ((q & 0xff) ^ 0x80) - 0x80
        d.append(lo)
        q = (q - lo) >> 8
    return d + [q]


def fix_exp(mx):
    """hb_fix_exp of max |r|: 53 - ilogb, 0 for the zero vector"""
    return 54 - math.frexp(mx)[1] if mx > 0 else 0


def quantise(r):
    """(E, q): q = rint(r 2^E) as int64 (exact: |q| < 2^54, asserted)"""
    E = fix_exp(float(np.abs(r).max()))
    qf = np.rint(np.ldexp(r, E))
    assert np.abs(qf).max() < 2.0 ** 54
    return E, qf.astype(np.int64)


def digit_planes(q):
    """digits_of for an int64 vector: HB_ND x len(q), int64"""
    q = np.array(q, dtype=np.int64)
    planes = np.zeros((HB_ND, len(q)), dtype=np.int64)
    for k in range(HB_ND - 1):
        lo = ((q & 0xff) ^ 0x80) - 0x80
        planes[k] = lo
        q = (q - lo) >> 8
    planes[HB_ND - 1] = q
    return planes


def limbs18(q):
    """q = l0 + l1 2^18 + l2 2^36 with 0 <= l0, l1 < 2^18 and |l2| <= 2^18: the split the exact product is taken over"""
    q = np.array(q, dtype=np.int64)
    l0 = q & 0x3ffff
    l1 = (q >> 18) & 0x3ffff
    l2 = q >> 36
    assert np.array_equal(l0 + (l1 << 18) + (l2 << 36), q) and np.abs(l2).max(initial=0) <= 2 ** 18
    return np.stack([l0, l1, l2])


def integer_products(X, V):
    """X' V' in exact integers (X: n x m int8, V: k x n int64 with |V| <= 2^18): float64 BLAS on chunks of 64 columns. Every partial sum
    is an integer of magnitude at most n max|x| max|v|, and that is asserted to lie below 2^53, so no addition rounds in any order."""
    n, m = X.shape
    xm = max(abs(int(X.min())), abs(int(X.max())))
    assert n * xm * int(np.abs(V).max(initial=0)) < 2 ** 53
    Vf = np.ascontiguousarray(V.T, dtype=np.float64)
    out = np.zeros((m, V.shape[0]), dtype=np.int64)
    for c0 in range(0, m, 64):
        s = X[:, c0:c0 + 64].astype(np.float64).T @ Vf
        assert np.array_equal(s, np.rint(s))
        out[c0:c0 + 64] = s.astype(np.int64)
    return out


def horner(acc, E):
    """hbq_finalize on the seven plane sums of one column, in integers: a = 0; a = float(int(a) 256 + acc_k) for k = 6 .. 0 (the correctly
    rounded fma); ldexp(a, -E). Returns (value, exact integer sum_k acc_k 256^k, R) with R the number of steps whose exact partial value
    reaches 2^53 — the steps that can round: every other one is exact."""
    a, p, R = 0.0, 0, 0
    for k in range(HB_ND - 1, -1, -1):
        a = float(int(a) * 256 + int(acc[k]))
        p = p * 256 + int(acc[k])
        R += abs(p) >= 2 ** 53
    return math.ldexp(a, -E), p, R


def ulps_off(value, exact, E):
    """|value - exact 2^-E| in ulps of the correctly rounded exact 2^-E; value 2^E is one of the recurrence's integers"""
    if exact == 0:
        return abs(value)
    a = math.ldexp(value, E)
    assert a == int(a)
    return abs(int(a) - exact) / float(np.spacing(abs(float(exact))))     # (float(int) rounds correctly; the scale 2^-E moves both alike)


def restate(X, r):
    """The device's dot products of the columns of X with r, restated: a dict with E, q, planes (HB_ND x n, int8 as the device holds them), acc (m x HB_ND int64 plane
    sums), d (m doubles, what every kernel must return bit for bit), exact (m Python integers, sum_i x_ij q_i from the 18-bit limbs),
    R (m) and ulps (m: the restatement's distance from the exact product in ulps — at most R / 2, asserted here)."""
    E, q = quantise(np.asarray(r, dtype=np.float64))
    planes = digit_planes(q)
    assert int(np.abs(planes[:HB_ND - 1]).max(initial=0)) <= 128 and int(np.abs(planes[HB_ND - 1]).max(initial=0)) <= 64
    both = integer_products(X, np.concatenate([planes, limbs18(q)]))
    acc, lim = both[:, :HB_ND], both[:, HB_ND:]
    m = X.shape[1]
    d, exact, R, ulps = np.zeros(m), [], np.zeros(m, dtype=np.int64), np.zeros(m)
    for j in range(m):
        d[j], p, R[j] = horner(acc[j], E)
        ex = int(lim[j, 0]) + (int(lim[j, 1]) << 18) + (int(lim[j, 2]) << 36)
        assert p == ex, (j, "the planes and the limbs recombine to different integers")
        exact.append(ex)
        ulps[j] = ulps_off(d[j], ex, E)
        assert ulps[j] <= R[j] / 2, (j, ulps[j], R[j])
    return {"E": E, "q": q, "planes": planes.astype(np.int8), "acc": acc, "d": d, "exact": exact, "R": R, "ulps": ulps}


# ------------------------------------------------------------------------------------------------------------------------
# the inputs of the tall tests
# ------------------------------------------------------------------------------------------------------------------------
SPECIAL2 = {"all 3": 1, "all 0": 2, "one 3 in the last row": 3, "3 from row 131072 on": 4}                   # columns of both layouts
SPECIAL8 = {"all 127": 5, "all -127": 6, "alternating +-127": 7, "all -128": 8}                               # int8 columns only


def tall_genotypes(n, m, seed):
    """(X2, X8): codes 0..3 by rand_geno3's recipe (three allele draws; a 3 at each of the 16 positions of column 0's first packed word,
    column 1 all 3) with the columns of SPECIAL2, and the same matrix with the columns of SPECIAL8 for the int8 context (m >= 64)."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.5, m).astype(np.float32)
    X = np.zeros((n, m), dtype=np.int8, order="F")
    for j in range(m):                                  # (column by column: n x m doubles at once would be 400 MB at the tallest size)
        X[:, j] = sum((rng.random(n, dtype=np.float32) < p[j]).astype(np.int8) for _ in range(3))
    X[:16, 0] = 3
    X[:, SPECIAL2["all 3"]] = 3
    X[:, SPECIAL2["all 0"]] = 0
    X[:, SPECIAL2["one 3 in the last row"]] = 0
    X[n - 1, SPECIAL2["one 3 in the last row"]] = 3
    if n > 131072:                                      # (at n = 131 072 there are no such rows: the column stays a random one)
        X[:131072, SPECIAL2["3 from row 131072 on"]] = 0
        X[131072:, SPECIAL2["3 from row 131072 on"]] = 3
    assert X.min() == 0 and X.max() == 3
    X8 = X.copy(order="F")
    X8[:, SPECIAL8["all 127"]] = 127
    X8[:, SPECIAL8["all -127"]] = -127
    X8[0::2, SPECIAL8["alternating +-127"]] = 127
    X8[1::2, SPECIAL8["alternating +-127"]] = -127
    X8[:, SPECIAL8["all -128"]] = -128
    return X, X8


def tall_residuals(n, seed):
    """name -> residual: the cases of the tall tests"""
    rng = np.random.default_rng(seed)
    out = {}
    r = rng.normal(0, 3.0, n)
    r[rng.choice(n, 5, replace=False)] *= 1e6
    out["normal, five rows x 1e6"] = r
    lo, hi = math.ldexp(float(Q_LOW), -53), math.ldexp(float(Q_HIGH), -53)
    assert int(math.ldexp(lo, 53)) == Q_LOW and int(math.ldexp(hi, 53)) == Q_HIGH
    out["every row at q_low"] = np.full(n, lo)
    r = np.full(n, lo)
    r[1::2] = -lo
    out["q_low, alternating signs"] = r
    r = np.full(n, hi)
    r[n // 3] = 1.0                                     # (the maximum: E = 53, and 2^53 has digits 0 .. 0, 32)
    out["one row at 1, the others at q_high"] = r
    out["zero"] = np.zeros(n)
    return out
