"""Inputs on which the control logic of the summary-level chain kernels (k_sb_group / k_sb_update, hb_sbayes.hpp; k_ss_group /
k_ss_update, hb_sbayes_sparse.hip) is CERTAIN to run — a helper for test_sbayes_rounds_host.py (which proves each regime from the
sequential reference's trace, tests/sbayess_restatement.py) and test_gpu_sbayes_rounds.py (which compares sweep by sweep), not a
test.

The samplers take the LD matrix and the summary statistics directly, so no genotypes are made: ldm = V * R with R the identity
plus a few small blocks (positive definite by construction), joint effects beta, the marginal column b = R beta with |b| < 1e-12
set to exactly 0, se = 1 / sqrt(n V), N = n = 2000. With B the driver's joint effect the blocks are

  pair(a, c, r)        beta[a] = B, beta[c] = -r B: the driver's marginal is B (1 - r^2), the second marker's exactly 0 — out of
                       the model when the sweep reaches its group and certain to be pushed in once the driver has moved: a CROSSER
                       (the round that passed over it has to be rolled back);
  cascade(a, a+1, a+2) R[a, a+1] = R[a+1, a+2] = r = 0.6, R[a, a+2] = 0, beta = B, -r B / (1 - r^2), r^2 B / (1 - r^2): both
                       followers have marginal 0 and the third crosses only after the second has moved — two rollbacks in a row;
  tag(a, a+1, r)       beta[a] = B, beta[a+1] = 0: the tag's marginal r B is over its threshold at entry and it is excluded once
                       the driver has moved: a LEAVER.

A group is GS = 512 consecutive markers (SB_GS = SS_GS) and a round holds at most ROUND = 64 candidates: facts of the kernels,
named here; nothing below simulates a round.

Every matrix comes in three forms: "dense" (ndarray), "full" (CSC with every entry stored, zeros included: nnz = m * m, varediff
= 0, the sparse sampler is then the dense one) and "nz" (CSC of the non-zeros: varediff is live, most columns hold the diagonal
alone)."""
import numpy as np
import scipy.sparse as sp

GS, ROUND = 512, 64
V, N_OBS = 0.4, 2000
RUN = dict(niter=3, nburn=0, thin=1)          # every sweep recorded: sweep 0 starts from g = 0, sweeps 1 and 2 have markers in

# the models of "rounds": (name, model, Pi, fold). Chosen on the CPU so that every regime of
# test_sbayes_rounds_host.py holds under SEED: BayesR's usual folds [0, 1e-4, 1e-3, 1e-2] leave 23 of the 70 drivers in at sweep
# 0, these leave all of them in. Seven classes make kpad = 7 (k_sb_group<7> / k_ss_group<7>).
ROUNDS_MODELS = [
    ("cpi", "BayesCpi", [0.95, 0.05], None),
    ("b", "BayesB", [0.95, 0.05], None),
    ("r4", "BayesR", [0.9, 0.04, 0.03, 0.03], [0, 1e-2, 1e-1, 1.0]),
    ("r7", "BayesR", [0.9, 0.02, 0.02, 0.02, 0.02, 0.01, 0.01], [0, 1e-3, 1e-2, 3e-2, 1e-1, 3e-1, 1.0]),
]
EVERYONE_MODELS = [("rr", "BayesRR", [0.95, 0.05], None), ("a", "BayesA", [0.95, 0.05], None), ("l", "BayesL", [0.95, 0.05], None)]
CPI = ("cpi", "BayesCpi", [0.95, 0.05], None)
SIZES = [1, 2, 63, 64, 65, 511, 512, 513]
SEED = 7


def full_csc(ld):
    """every entry stored, exact zeros included"""
    m = ld.shape[0]
    return sp.csc_matrix((np.asfortranarray(ld).ravel(order="F").copy(), np.tile(np.arange(m, dtype=np.int32), m),
                          np.arange(0, m * m + 1, m, dtype=np.int64)), shape=(m, m))


def _case(R, beta, nan=()):
    m = R.shape[0]
    assert np.array_equal(R, R.T)
    ldm = V * R
    b = R @ beta                                           # = (ldm @ beta) / V
    b[np.abs(b) < 1e-12] = 0.0
    b[list(nan)] = np.nan
    ss = np.column_stack([np.full(m, 0.3), b, np.full(m, 1.0 / np.sqrt(N_OBS * V)), np.full(m, float(N_OBS))])
    nz = sp.csc_matrix(ldm)
    nz.sort_indices()
    full = full_csc(ldm)
    assert full.nnz == m * m and nz.nnz == np.count_nonzero(ldm)
    return {"m": m, "ss": ss, "dense": ldm, "full": full, "nz": nz}


def _pair(R, beta, a, c, B, r=0.8):
    R[a, c] = R[c, a] = r
    beta[a], beta[c] = B, -r * B


def _cascade(R, beta, a, B, r=0.6):
    R[a, a + 1] = R[a + 1, a] = R[a + 1, a + 2] = R[a + 2, a + 1] = r
    beta[a], beta[a + 1], beta[a + 2] = B, -r * B / (1 - r * r), r * r * B / (1 - r * r)


def _late_cascade(R, beta, a, B, r=0.6):
    """the cascade with its driver LAST (a + 2), linked to a, which is linked to a + 1: in sweep 0 the driver alone moves; in sweep 1
    marker a is a candidate at entry and its move pushes a + 1 in — a crosser in a sweep that began with markers in the model"""
    R[a + 2, a] = R[a, a + 2] = R[a, a + 1] = R[a + 1, a] = r
    beta[a + 2], beta[a], beta[a + 1] = B, -r * B / (1 - r * r), r * r * B / (1 - r * r)


def _tag(R, beta, a, B, r=0.8):
    R[a, a + 1] = R[a + 1, a] = r
    beta[a] = B


ROUNDS_SECOND = np.arange(1, 140, 2)                       # the second markers of the 70 pairs at 0..139
ROUNDS_NAN = (149, 512, 700)


def rounds():
    """m = 1100: two full groups and a tail of 76. Group 0 holds more than 64 candidates at entry AND more than 64 moves (several
    rounds, each fold in more than one chunk of SB_CH = 32, k_sb_update in more than one chunk of 64) with a crosser in nearly
    every pair; the cascade at 300..302; the cascade with its driver last at 210..212 (a crosser in sweep 1); the tag at 400; a crosser that is its group's last marker (511) and one that is the last
    marker of the ragged tail (1099); a pair across a group edge (1023, 1024) and one across a whole group (150, 1050), whose
    second markers are pushed in by the update kernel before their own group starts; markers without statistics."""
    m = 1100
    R, beta = np.eye(m), np.zeros(m)
    for a in range(0, 140, 2):
        _pair(R, beta, a, a + 1, 0.5)
    _cascade(R, beta, 300, 1.5)
    _late_cascade(R, beta, 210, 1.5)
    _tag(R, beta, 400, 0.5)
    for a, c in ((510, 511), (1023, 1024), (1098, 1099), (150, 1050)):
        _pair(R, beta, a, c, 0.5)
    return _case(R, beta, ROUNDS_NAN)


def everyone():
    """m = 513, one full group and a tail of one marker, ldm = V * 0.5 ** |i - j|, for the models in which every marker moves in
    every sweep: 510 moves in the full group (markers 0 and 511 have no statistics), eight rounds of 64."""
    m = 513
    d = np.abs(np.subtract.outer(np.arange(m), np.arange(m)))
    R = 0.5 ** d
    b = np.random.default_rng(11).normal(0, 0.1, m)
    b[[0, 511]] = np.nan
    ss = np.column_stack([np.full(m, 0.3), b, np.full(m, 1.0 / np.sqrt(N_OBS * V)), np.full(m, float(N_OBS))])
    ldm = V * R
    nz = sp.csc_matrix(ldm)
    nz.sort_indices()
    return {"m": m, "ss": ss, "dense": ldm, "full": full_csc(ldm), "nz": nz}


def size(m):
    """a pair at (m - 2, m - 1) — the last marker is a crosser — behind strong single markers: all of 0 .. m - 3 where m <= 65 (so
    that a round is exactly full at m = 64 and one over at m = 65), the first 40 and every 7th beyond that"""
    R, beta = np.eye(m), np.zeros(m)
    singles = range(m - 2) if m <= 65 else [j for j in range(m - 2) if j < 40 or j % 7 == 0]
    for j in singles:
        beta[j] = 0.5 if j % 2 else -0.5
    if m >= 2:
        _pair(R, beta, m - 2, m - 1, 0.5)
    else:
        beta[0] = 0.5
    return _case(R, beta)


def empty_group():
    """m = 1030: group 1 (512..1023) has no marker with statistics, so it must leave no move behind for the update kernel; group
    0 moves before it and the tail's pair (1024, 1025) has its crosser after it"""
    m = 1030
    R, beta = np.eye(m), np.zeros(m)
    _pair(R, beta, 100, 101, 0.5)
    _pair(R, beta, 1024, 1025, 0.5)
    return _case(R, beta, range(512, 1024))


def derive(rec):
    """what the tests read off one sweep's trace record (all from the sequential reference)"""
    gb = rec["g_before"]
    cand = rec["entry_in"] | (gb != 0)
    return {"cand_entry": cand, "crosser": ~cand & rec["turn_in"], "leaver": cand & (gb == 0) & ~rec["turn_in"],
            "left_model": (gb != 0) & ~rec["turn_in"], "moved": rec["moved"]}


def per_group(x, m):
    """counts of a boolean m-vector per group of GS"""
    return [int(x[g0:g0 + GS].sum()) for g0 in range(0, m, GS)]
