"""From plan to launch: every mat-vec launch of a sweep has the blocks that hb_matvecplan.hpp states.

tests/test_host_logic.py checks plan_matvec against tests/golden/matvec_plan_table.json without a device. It cannot see whether the
launcher (launch_dotq, hb_kernels.hip) applies the answer. Here one sweep runs with block stamps on (set_profiling(8)): each launch
records the block count it was given, and each of its blocks the clock at its start. Both are compared with the record."""
import ctypes as ct

import numpy as np
import pytest

import hibayes_amd as H
from run_plan_record import recorded_matvec_plan

pytestmark = pytest.mark.gpu

STAMP_BLOCKS = 4608   # HB_LSTAMP_BLOCKS
# (stage of the record, the knobs' defaults as its key prefix) by (layout, mat-vec kind)
FAMILY = {(8, None): ("dotq", "768"), (2, 2): ("dotq2m", "1 0 4 0"), (2, 0): ("dotq2", "1 256 1600"), (2, 1): ("dotq2r", "16")}


@pytest.fixture(scope="module")
def plan():
    return recorded_matvec_plan()


@pytest.fixture(scope="module")
def num_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _launch_blocks(c, g):
    """(blocks launch g of the last sweep was given, the start stamps of its blocks)"""
    c.L.hb_ctx_debug_launch_stamps.argtypes = [ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_int, ct.c_void_p]
    buf, nb = np.zeros(2 * STAMP_BLOCKS, dtype=np.uint64), ct.c_int()
    H._lib.check(c.L.hb_ctx_debug_launch_stamps(c.h, g, buf.ctypes.data, STAMP_BLOCKS, ct.byref(nb)))
    return nb.value, buf[:2 * nb.value:2]


def _one_sweep_against_the_record(c, plan, num_cus, model, Lv, D, layout, kind, dense):
    stage, knobs = FAMILY[(layout, kind)]
    P, ld = c.panel, c.ld
    npanels = -(-c.m // P)
    ngroups = -(-npanels // D)
    c.set_profiling(0)
    c.set_profiling(8)   # (fresh stamps, all zero)
    c.sweep(model, 0, 0.5, 0.01, logpi=np.log([0.95, 0.05]), fold=[0, 0])
    for g in range(ngroups):
        ncols = (min(npanels, (g + 1) * D) - g * D) * P
        # the riders the pipeline gives launch g: the update rows of group g - Lv, the finalize rows of launch g - 1 (D panels wide)
        upd = 0 if g < Lv else 2 if dense else 1
        fin = 0 if g == 0 else {ncols: 2, 2 * ncols: 3}[D * P]
        nupd, nfin = (0, ld // 256, ld // 64)[upd], (D * P // 64 if g else 0)
        kernel, _, ncg, _, _, trows = plan[stage]["%s %d %d %d %d %d" % (knobs, ld, ncols, num_cus, upd, fin)].split()
        want = nupd + nfin + int(ncg) * int(trows)
        got, starts = _launch_blocks(c, g)
        what = "%s, layout %d kind %s, ld %d, launch %d of %d (%d columns, %d update + %d finalize rows, %s)" % (model, layout, kind, ld, g, ngroups, ncols, nupd, nfin, kernel)
        assert got == want, "%s: %d blocks, the record has %d" % (what, got, want)
        assert np.all(starts != 0), "%s: %d of its %d blocks left no start stamp" % (what, int((starts == 0).sum()), got)
    assert _launch_blocks(c, ngroups)[0] == 0


def _context(n, m, P, Lv, D):
    c = H.Context(n, m, panel=P, seed=20261018)
    c.generate(20261018, mono_every=97)
    rng = np.random.default_rng(n + m)
    c.set_residual(rng.normal(0, 1, n), np.zeros(n))
    c.set_pipeline(1, Lv, D)
    assert c.pipeline()[:3] == (1, Lv, D)
    c.build_gram()
    return c


# m = 4608 at panel 512, geometry (2, 2): five launches, the last one panel wide; m = 1100 at panel 128, (2, 1): nine launches over ragged markers
@pytest.mark.parametrize("m,P,Lv,D", [(4608, 512, 2, 2), (1100, 128, 2, 1)])
@pytest.mark.parametrize("n", [300, 700, 1300])   # ld 512; 768: the 512-individual shapes fall back; 1536
def test_every_launch_of_a_sweep_has_the_blocks_the_record_states(plan, num_cus, n, m, P, Lv, D):
    """One BayesCpi sweep on int8 columns (k_dotq), then on 2-bit columns with each of the three kernels (k_dotq2m, k_dotq2, k_dotq2r):
    the block count every launch was given equals update + finalize + tiles of the recorded plan for the launch's width and riders, and
    every one of those blocks ran."""
    assert num_cus in (32, 64, 256), "the record has no row for %d compute units" % num_cus
    with _context(n, m, P, Lv, D) as c:
        assert c.ld == -(-n // 256) * 256
        _one_sweep_against_the_record(c, plan, num_cus, "BayesCpi", Lv, D, 8, None, False)
        c.set_layout(2, keep_int8=True)
        for kind in (2, 0, 1):
            c.set_matvec_kernel(kind)
            _one_sweep_against_the_record(c, plan, num_cus, "BayesCpi", Lv, D, 2, kind, False)


def test_dense_update_rows_ride_with_their_own_block_count_and_lds(plan, num_cus):
    """BayesRR at panel 512, geometry (2, 2), int8 columns: the update rows that ride in the launches are the dense ones, ld / 64 of them
    (k_dotq is then launched with HBU_LDS), and the last launch finalizes a launch twice its width."""
    assert num_cus in (32, 64, 256)
    with _context(700, 4608, 512, 2, 2) as c:
        _one_sweep_against_the_record(c, plan, num_cus, "BayesRR", 2, 2, 8, None, True)
