"""The 512-individual shapes of the matrix-core mat-vec (k_dotq2m<4, 0, *> and <4, 3, *>, hb_dotq2.hpp: dotq2m512_tile) keep a ring of
genotype stage buffers in LDS and a ring of digit registers beside it, several stages requested ahead and waited for by count. What can go
wrong in such a ring depends on how many stages a tile has: the prologue requests min(depth - 1, stages), the steady state one more per
stage multiplied, the drain lets 2, 1, 0 stages stay outstanding, and the slot a stage lives in is its number modulo the depth. The cases
below are the smallest that take every such path of a ring three or four deep (three is built), on residuals whose digit planes sit at the edges of int8, compared
bit for bit with the int8 layout's kernel (the same integers summed in another order) and, once, with the Python big-integer product."""
import numpy as np
import pytest

import hibayes_amd as H
from test_gpu_kernels import _digit_edge_residuals, rand_geno, rand_geno3

pytestmark = pytest.mark.gpu

# individuals -> 512-individual stages of a column (the padded length is ceil(n / 256) * 256): 1, 2, 3, 4, 5 and 9 stages. With HB_DOTQ2_TILES
# beyond what the plan accepts, a column is cut into as many tiles as plan_matvec allows — at most a quarter of its stages: one tile up to
# seven stages, and the nine-stage column into tiles of 5 and 4 (full prologue, steady state, the whole drain; the second tile starts at
# stage 5). n = 1200 pads to 1280, no multiple of 512: the plan falls back to the 256-individual shape, the control that this file's
# harness itself agrees with the int8 kernel.
STAGES = {500: 1, 1000: 2, 1500: 3, 2000: 4, 2500: 5, 4600: 9, 1200: None}
WIDTHS = ((64, 64), (512, 512), (1024, 512))   # (columns, panel): one column group, one panel, two panels
SHAPES = [{}, {"HB_Q2M_SC": "0"}, {"HB_Q2M_G": "3"}, {"HB_Q2M_G": "3", "HB_Q2M_SC": "0"}]
MAKERS = {"codes 0..2": rand_geno, "codes 0..3": rand_geno3}

_inputs = {}


def inputs(maker, n, m, panel):
    """Genotypes, the digit-edge residuals and the int8 layout's dot products for them: made once, shared by every shape, never written to."""
    key = (maker, n, m)
    if key not in _inputs:
        rng = np.random.default_rng([n, m, len(maker)])
        X = MAKERS[maker](rng, n, m)
        res = _digit_edge_residuals(n, rng)
        want = {}
        with H.Context(n, m, panel=panel, precise=2) as c:
            c.upload(X)
            for name, r in res.items():
                c.set_residual(r, np.zeros(n))
                want[name] = c.dot().copy()
        for a in [X, *res.values(), *want.values()]:
            a.setflags(write=False)
        _inputs[key] = (X, res, want)
    return _inputs[key]


def test_the_cases_have_the_stage_counts_they_are_named_for():
    for n, st in STAGES.items():
        ld = (n + 255) // 256 * 256
        assert (ld % 512 == 0 and ld // 512 == st) if st else ld % 512 != 0


@pytest.mark.parametrize("maker", list(MAKERS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: ",".join("%s=%s" % kv for kv in s.items()) or "default")
def test_every_prologue_steady_state_and_drain_of_the_stage_ring(shape, maker, monkeypatch):
    """Every tile length 1..5 and the 5 + 4 split, at 64, 512 and 1024 columns, in both accumulator forms and both lane orders, on genotypes
    with and without code 3: the 2-bit matrix-core kernel returns the int8 kernel's doubles bit for bit."""
    monkeypatch.setenv("HB_DOTQ2_TILES", "100000")
    for k, v in shape.items():
        monkeypatch.setenv(k, v)
    for n in STAGES:
        for m, panel in WIDTHS:
            X, res, want = inputs(maker, n, m, panel)
            with H.Context(n, m, panel=panel, precise=2) as c:
                c.upload(X)
                c.set_layout(2, keep_int8=False)
                c.set_matvec_kernel(2)
                for name, r in res.items():
                    c.set_residual(r, np.zeros(n))
                    got = c.dot()
                    assert np.array_equal(got.view(np.uint64), want[name].view(np.uint64)), (shape, maker, n, m, name)


def test_the_stage_ring_against_the_big_integer_product(monkeypatch):
    """Five stages (prologue, steady stages, the whole drain) of code-3 genotypes against the exact product of the genotypes with
    q = rint(r 2^E), E = 53 - ilogb(max |r|), scaled back: correctly rounded while the exact sum stays below 2^61, within one ulp from there
    on (hbq_finalize's Horner recurrence: see test_gpu_kernels.test_quantiser_and_finalize_at_the_digit_edges)."""
    monkeypatch.setenv("HB_DOTQ2_TILES", "100000")
    n, m = 2500, 64
    X, res, _ = inputs("codes 0..3", n, m, 64)
    Xo = X.astype(object).T
    with H.Context(n, m, panel=64, precise=2) as c:
        c.upload(X)
        c.set_layout(2, keep_int8=False)
        c.set_matvec_kernel(2)
        for name, r in res.items():
            c.set_residual(r, np.zeros(n))
            d = c.dot()
            mx = np.abs(r).max()
            E = 54 - int(np.frexp(mx)[1]) if mx > 0 else 0
            q = np.rint(np.ldexp(r, E))
            exact = Xo @ np.array([int(v) for v in q], dtype=object)
            want = np.array([np.ldexp(float(v), -E) for v in exact])
            small = np.array([abs(v) < 2 ** 61 for v in exact])
            assert np.array_equal(d[small], want[small]), name
            assert (np.abs(d[~small] - want[~small]) <= np.spacing(np.abs(want[~small]))).all(), name
