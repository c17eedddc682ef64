"""Host-side pieces of the product that need no GPU: loaders, formula handling, windows, sharding."""
import os

import numpy as np
import pytest

import hibayes_amd as H
from hibayes_amd import bayes as B
from hibayes_amd.dist import shard_range
from oracle import oracle as O


def test_product_bed_decoder_equals_oracle_and_readme(demo):
    raw = open(demo["prefix"] + ".bed", "rb").read()
    g = H.decode_bed(raw, 600, 1000)
    assert g.flags["F_CONTIGUOUS"] and g.dtype == np.int8
    assert np.array_equal(g, O.decode_bed(raw, 600, 1000))
    assert g[:4, :5].tolist() == [[2, 1, 1, 1, 0], [1, 0, 1, 1, 0], [0, 2, 0, 0, 0], [1, 1, 1, 1, 0]]


def test_decoder_ragged_missing_dominance():
    rng = np.random.default_rng(5)
    nind, nsnp = 13, 7  # nind not a multiple of 4: last byte of each SNP is ragged
    bpc = (nind + 3) // 4
    body = rng.integers(0, 256, size=nsnp * bpc, dtype=np.uint8)
    raw = bytes([0x6C, 0x1B, 0x01]) + body.tobytes()
    for imp in (False, True):
        assert np.array_equal(H.decode_bed(raw, nind, nsnp, impute=imp), O.decode_bed(raw, nind, nsnp, impute=imp))
    d = H.decode_bed(raw, nind, nsnp, impute=True, mode="D")
    assert set(np.unique(d)) <= {0, 1}
    with pytest.raises(ValueError):
        H.decode_bed(b"\x00\x00\x00" + body.tobytes(), nind, nsnp)
    with pytest.raises(ValueError):
        H.decode_bed(raw[:10], nind, nsnp)


def test_read_plink_writes_bigmemory_style_bin(tmp_path, demo):
    out = str(tmp_path / "demo_out")
    d = H.read_plink(demo["prefix"], out=out)
    assert len(d["fam"]) == 600 and len(d["map"]["SNP"]) == 1000
    raw = np.fromfile(out + ".bin", dtype=np.int8)
    assert raw.size == 600 * 1000
    assert np.array_equal(raw.reshape(1000, 600).T, d["geno"])  # column-major on disk
    assert open(out + ".id").read().split()[:2] == ["IND0701", "IND0702"]


def test_ibrm_alignment_matches_reference_rules(demo):
    # R/bayes.r:161-165 and :199-207: 600 genotyped, 500 phenotyped, 300 shared with a T1 record
    assert len(demo["rows"]) == 300
    assert demo["y"].mean() == pytest.approx(24.548275, rel=1e-9)
    assert demo["y"].var(ddof=1) == pytest.approx(215.2144812894398, rel=1e-12)


def test_model_matrix_treatment_contrasts():
    cols = {"season": ["Winter", "Spring", "Summer", "Spring"], "bwt": ["1.5", "2", "3", "1"]}
    X, names = B._model_matrix(cols, ["season", "bwt"], [0, 1, 2, 3])
    assert names == ["seasonSummer", "seasonWinter", "bwt"]
    assert X[:, 0].tolist() == [0, 0, 1, 0] and X[:, 1].tolist() == [1, 0, 0, 0] and X[:, 2].tolist() == [1.5, 2, 3, 1]


def test_cutwind_matches_bruteforce_restatement():
    rng = np.random.default_rng(2)
    chrom = np.repeat([1, 2, 3], [40, 25, 7])
    pos = np.concatenate([np.sort(rng.integers(1, 5000, 40)), np.sort(rng.integers(1, 3000, 25)), np.arange(1, 8)]).astype(float)
    w = H.cutwind_by_num(chrom, pos, 10)
    # src/cutwind.cpp:40-65: windows of 10 in position order per chromosome; short chromosomes form one window
    assert w.min() == 1 and w.max() == 4 + 3 + 1
    for c in (1, 2):
        idx = np.flatnonzero(chrom == c)
        assert np.all(np.diff(w[idx][np.argsort(pos[idx], kind="stable")]) >= 0)
    assert len(set(w[chrom == 3])) == 1
    wb = H.cutwind_by_bp(chrom, pos, 1000.0)
    for c in (1, 2, 3):
        idx = np.flatnonzero(chrom == c)
        bins = np.floor((pos[idx] - 1) / 1000.0)
        # same bin <=> same window (src/cutwind.cpp:14-35)
        for i in range(idx.size):
            for j in range(idx.size):
                assert (bins[i] == bins[j]) == (wb[idx[i]] == wb[idx[j]])


def test_shard_ranges_tile_markers_contiguously():
    for m, w in ((1000, 8), (1003, 8), (7, 8), (500000, 3)):
        lo_prev = 0
        for r in range(w):
            lo, hi = shard_range(m, r, w)
            assert lo == lo_prev and hi >= lo
            lo_prev = hi
        assert lo_prev == m
        sizes = [shard_range(m, r, w)[1] - shard_range(m, r, w)[0] for r in range(w)]
        assert max(sizes) - min(sizes) <= 1


def test_product_fails_loudly_without_gpu():
    if H.lib().hb_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(H.HibayesError) as ei:
        H.Context(10, 10)
    assert ei.value.status == 2 and "no CPU fallback" in str(ei.value)
    with pytest.raises(H.HibayesError):
        H.Bayes(np.arange(10.0), np.ones((10, 4), dtype=np.int8), "BayesCpi", [0.95, 0.05], niter=2, nburn=0, thin=1)


def test_bigmemory_backing_files_round_trip(tmp_path, demo):
    """read_plink(out=) leaves xx.bin / xx.desc / xx.id / xx.map (reference R/read_plink.r:39-75); a later session
    re-attaches them (attach.big.matrix) and hands the int8 matrix to ibrm() without a double copy."""
    import hibayes_amd as H
    out = str(tmp_path / "demo_out")
    pl = H.read_plink(demo["prefix"], out=out)
    assert os.path.getsize(out + ".bin") == 600 * 1000
    bm = H.read_bigmatrix(out)
    assert bm["geno"].dtype == np.int8 and bm["geno"].shape == (600, 1000) and bm["geno"].flags["F_CONTIGUOUS"]
    assert np.array_equal(np.asarray(bm["geno"]), pl["geno"])
    assert bm["geno"][:4, :5].tolist() == [[2, 1, 1, 1, 0], [1, 0, 1, 1, 0], [0, 2, 0, 0, 0], [1, 1, 1, 1, 0]]   # README.md:81-86
    assert bm["id"] == [r[1] for r in pl["fam"]]
    assert bm["map"]["SNP"] == pl["map"]["SNP"] and np.array_equal(bm["map"]["Pos"], pl["map"]["Pos"])
    # the .map keeps the .bim's position text (rMap_c writes strings): 9-digit positions survive
    assert open(out + ".map").readline() == "SNP\tCHROM\tPOS\tA1\tA2\n"


def test_bigmemory_descriptor_as_r_prints_it(tmp_path):
    import hibayes_amd as H
    from hibayes_amd.plink import parse_bigmatrix_desc
    # dput() of a big.matrix.descriptor as bigmemory writes it (line breaks where deparse() puts them)
    desc = ('new("big.matrix.descriptor", description = list(sharedType = "FileBacked", \n'
            '    filename = "g.bin", dirname = "/somewhere/else/", totalRows = 7L, \n'
            '    totalCols = 5L, rowOffset = c(0, 7), colOffset = c(0, \n'
            '    5), nrow = 7, ncol = 5, rowNames = NULL, colNames = NULL, \n'
            '    type = "char", separated = FALSE))\n')
    d = parse_bigmatrix_desc(desc)
    assert (d["totalRows"], d["totalCols"], d["type"], d["filename"], d["separated"]) == (7, 5, "char", "g.bin", False)
    g = (np.arange(35, dtype=np.int16).reshape(7, 5) % 3).astype(np.int8)
    g[2, 3] = -128                                   # NA_CHAR
    g.T.tofile(str(tmp_path / "g.bin"))              # column-major bytes, as the mmap holds them
    (tmp_path / "g.desc").write_text(desc)
    m = H.attach_bigmatrix(str(tmp_path / "g.desc"))  # the recorded dirname does not exist: found next to the .desc
    assert np.array_equal(np.asarray(m), g) and m[2, 3] == -128
    # a sub-matrix descriptor (rows 2..5, columns 1..3)
    (tmp_path / "s.desc").write_text(desc.replace("rowOffset = c(0, 7)", "rowOffset = c(2, 4)").replace("c(0, \n    5)", "c(1, \n    3)"))
    assert np.array_equal(np.asarray(H.attach_bigmatrix(str(tmp_path / "s.desc"))), g[2:6, 1:4])
    with pytest.raises(ValueError):
        parse_bigmatrix_desc("list(a = 1)")


def test_map_argument_of_ibrm_is_validated_like_the_reference(demo):
    from hibayes_amd.bayes import _map_columns
    mp = demo["plink"]["map"]
    chrom, pos = _map_columns(mp)                     # the loader's own dict (keys Chr / Pos)
    assert chrom.size == 1000 and pos.dtype == np.float64
    tab = np.array([["s1", "1", "100"], ["s2", "X", "123456789"], ["s3", "2", "7"], ["s4", "Y", "9"], ["s5", "X", "11"]], dtype=object)
    chrom, pos = _map_columns(tab)                    # R/bayes.r:237-243: X, Y numbered after the largest numeric chromosome
    assert chrom.tolist() == [1, 3, 2, 4, 3] and pos.tolist() == [100, 123456789, 7, 9, 11]
    for bad, msg in ((np.array([["s", "0", "5"]], dtype=object), "0 is not allowed in chromosome."),
                     (np.array([["s", "1", "0"]], dtype=object), "0 is not allowed in physical position."),
                     (np.array([["s", None, "5"]], dtype=object), "NAs are not allowed in chromosome."),
                     (np.array([["s", "1", "abc"]], dtype=object), "Characters are not allowed in physical position."),
                     (np.array([["s", "1"]], dtype=object), "At least 3 columns in map.")):
        with pytest.raises(ValueError, match=msg):
            _map_columns(bad)
    with pytest.raises(ValueError, match="map information must be provided."):
        _map_columns(None)


def test_bench_gpus_n_starts_n_ranks_by_itself():
    """`python bench.py --gpus 2` with no launcher around it must run two ranks (one process per GPU, torch.distributed rendezvous on
    127.0.0.1) and print ONE JSON line with n_gpus = 2 — north_star asks for sweeps/s at 1, 2, 4 and 8 GPUs."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo", "--m", "20000", "--dry-run"],
                       env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["ranks_counted_by_all_reduce"] == 2 and "2 ranks" in out["config"]["collective"]
    # and one rank stays one process: no launcher, no rendezvous
    p1 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--dry-run"], env=env, capture_output=True, text=True, timeout=120)
    assert p1.returncode == 0 and json.loads([ln for ln in p1.stdout.splitlines() if ln.startswith("{")][0])["n_gpus"] == 1


def test_sbrm_host_checks_before_any_device_work():
    """sbrm()'s own argument handling (reference R/sbayes.r:126-187): refused inputs say why without touching a device."""
    import scipy.sparse as sp
    from hibayes_amd.sbayes import sbrm
    ss = np.zeros((5, 8))
    ld = np.eye(5)
    with pytest.raises(NotImplementedError, match="sparse ldm"):
        sbrm(ss, sp.csc_matrix(ld), "BayesCpi")
    with pytest.raises(NotImplementedError, match="CG"):
        sbrm(ss, ld, "CG")
    with pytest.raises(ValueError, match="can not implement GWAS analysis for the method: BayesRR"):
        sbrm(ss, ld, "BayesRR", windsize=1e6)
    with pytest.raises(ValueError, match="map information must be provided"):
        sbrm(ss, ld, "BayesCpi", windnum=2)
    mp = np.array([["s%d" % i, "1", str(100 * (i + 1))] for i in range(5)], dtype=object)
    with pytest.raises(ValueError, match="larger than the total number of markers"):
        sbrm(ss, ld, "BayesCpi", map=mp, windnum=9)
    with pytest.raises(ValueError, match="smaller than wind size"):
        sbrm(ss, ld, "BayesCpi", map=mp, windsize=1e6)
    with pytest.raises(ValueError, match="bad setting for collecting frequency"):
        sbrm(ss, ld, "BayesCpi", niter=10, nburn=8, thin=5)


def test_bench_line_stays_small_enough_for_the_driver_to_parse():
    """Round 5's bench line was 23 KB and the driver's record came back unparsed (`parsed: null`): the line is now built by
    bench.compact_line() from the full record, which goes to a file. Built here from round 5's full record (canned numbers):
    under 6000 bytes, one line, the contract's keys, ONE roofline and ONE cpu_baseline block of scalars, small side legs."""
    import json
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = json.load(open(os.path.join(root, "profiles", "r05_bench_driver_args.json")))
    res["roofline"].update(measured_copy_GBps=6290.0, frac_of_measured_copy=0.52)
    res["cpu_baseline"].update(int8_value=0.5, int8_cores=16)
    line = bench.compact_line(res, "profiles/bench_last_full.json")
    assert len(line) < bench.LINE_LIMIT <= 6000 and "\n" not in line
    out = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in out, k
    assert out["value"] == pytest.approx(res["value"], rel=1e-5) and out["config"]["workload"] and "model" in out["config"]
    assert all(not isinstance(v, (dict, list)) for v in out["roofline"].values())
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "bytes_per_launch", "avg_launch_ms", "measured_copy_GBps", "frac_of_measured_copy"):
        assert k in out["roofline"], k
    assert all(not isinstance(v, (dict, list)) for v in out["cpu_baseline"].values())
    for k in ("value", "unit", "cores", "kind", "sample", "value_1thread", "int8_value"):
        assert k in out["cpu_baseline"], k
    assert len(out["cpu_baseline"]["sample"]) <= 100
    assert {lg["leg"] for lg in out["legs"]} >= {"int8", "vdot4", "secondary", "all_move"}
    assert all(set(lg) <= {"leg", "model", "bits", "kernel", "value", "ms_per_step", "frac", "frac_sweep", "frac_of_measured_copy", "regime", "error"} for lg in out["legs"])
    # a sharded run adds its per-rank figures and the strong-scaling leg, still under the limit
    res.update(n_gpus=8, per_rank_ms_per_step={"min": 2.1, "max": 2.3, "all": [2.2] * 8}, ranks_counted_by_all_reduce=8,
               allreduce={"ms_per_call_back_to_back": 0.05, "bytes": 400128}, strong={"value": 900.0, "m_global": 2000000, "m_per_gpu": 250000, "ms_per_step": 4.4, "model": "BayesCpi"})
    out8 = json.loads(bench.compact_line(res, "x"))
    assert out8["strong_value"] == 900.0 and out8["ranks_counted_by_all_reduce"] == 8 and out8["per_rank_ms_per_step"]["max"] == 2.3 and out8["allreduce"]["ms_per_call"] == 0.05


def test_plain_bench_line_holds_the_contract_without_the_full_blocks():
    """A plain `bench.py` run (no --full) measures the headline only: its line still carries the contract's keys, and no roofline, regime,
    side legs, CPU baseline or full-record path (those need --full)."""
    import json
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    full = json.load(open(os.path.join(root, "profiles", "r05_bench_driver_args.json")))
    res = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                                "dtype", "data", "config", "achieved_GBps", "achieved_frac_of_hbm_peak")}
    out = json.loads(bench.compact_line(res, None))
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert out[k] == res[k], k
    assert out["value"] == pytest.approx(res["value"], rel=1e-5) and out["ms_per_step"] == pytest.approx(res["ms_per_step"], rel=1e-5)
    assert not {"roofline", "regime", "legs", "cpu_baseline"} & set(out) and out["full"] is None
    import sys
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--steps", "7", "--warmup", "3"]
        a = bench.parse()
        assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, "")
        sys.argv = ["bench.py", "--full", "--dump-outputs", "d"]
        a = bench.parse()
        assert a.full and a.dump_outputs == "d"
    finally:
        sys.argv = argv


def test_bench_dump_outputs_writes_float64_arrays(tmp_path, monkeypatch):
    """bench.py --dump-outputs: the effects, the residual and the hyper-parameters of the last timed step, float64 .npy each; an array
    above the cap becomes the same seeded sample every time."""
    import bench
    from hibayes_amd._lib import RunInfo

    class Ctx:
        def get_effects(self):
            return np.arange(10.0), np.zeros(10, dtype=np.uint8), np.zeros(10)

        def get_residual(self):
            return np.linspace(-1.0, 1.0, 4), np.zeros(4)

    info = RunInfo()
    info.mu, info.vare, info.varg, info.vara, info.nnz = 1.5, 2.0, 0.25, 0.0, 3.0
    info.pi[0], info.pi[1] = 0.9, 0.1
    bench.dump_outputs(str(tmp_path / "a"), Ctx(), info, 2, 5)
    got = {f[:-4]: np.load(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))}
    assert set(got) == {"alpha", "residual", "mu", "vare", "varg", "vara", "nnz", "pi"}
    assert all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["alpha"], np.arange(10.0)) and got["residual"].shape == (4,)
    assert got["mu"].tolist() == [1.5] and got["nnz"].tolist() == [3.0] and got["pi"].tolist() == [0.9, 0.1]
    monkeypatch.setattr(bench, "DUMP_CAP", 6)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), Ctx(), info, 2, 5)
    idx = np.load(str(tmp_path / "b" / "alpha_index.npy"))
    assert idx.size == 6 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(str(tmp_path / "b" / "alpha.npy")), idx)          # alpha[i] == i here
    assert np.array_equal(np.load(str(tmp_path / "c" / "alpha.npy")), np.load(str(tmp_path / "b" / "alpha.npy")))
    assert not os.path.exists(str(tmp_path / "b" / "residual_index.npy"))


def test_hot_kernels_are_built_without_register_spills():
    """The compiler's per-kernel resource report of the last build (hibayes_amd/csrc/hb_kernels.res.txt, written by the Makefile).
    The headline chain kernel sits at the 256-register limit of a 512-thread workgroup: in round 6 five spilled registers — caused by nothing
    more than other instantiations being added to the translation unit — cost 446 -> 421 sweeps/s without any test noticing."""
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hibayes_amd", "csrc", "hb_kernels.res.txt")
    if not os.path.exists(path):
        pytest.skip("no resource report: the library was not built by the Makefile here")
    rows, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", line)
        if m and cur:
            rows[cur][m.group(1).replace(" ", "")] = int(m.group(2))
    hot = {
        "headline chain (BayesB / BayesC, wide certified groups)": "_Z13k_chain_groupILi1ELi8ELi7ELi4ELb1E",
        "BayesR group chain": "_Z13k_chain_groupILi3ELi2ELi2ELi15ELb1E",
        "2-bit matrix-core mat-vec": "_Z8k_dotq2mILi4E",
        "int8 mat-vec": "_Z6k_dotq7dq_view",
    }  # (k_chain_dense does spill — 11 registers, 28 bytes —, has since round 4, and only outside its sub-block loop: eleven scratch instructions at the head and the tail of the panel loop)
    for what, prefix in hot.items():
        found = [k for k in rows if k.startswith(prefix)]
        assert found, "kernel missing from the report: %s (%s)" % (what, prefix)
        for k in found:
            assert rows[k].get("ScratchSize", 0) == 0 and rows[k].get("VGPRsSpill", 0) == 0, "%s spills: %s %s" % (what, k, rows[k])


_PLAN_PROGRAM = r"""
#include "hb_plan.hpp"
#include <cstdio>
#define G(a, b, c, d, e) printf("table group<%d,%d,%d,%d,%d>\n", a, b, c, d, e);
#define P(a, b) printf("table persist<%d,%d>\n", a, b);
#define D(a) printf("table dense<%d>\n", a);
#define F(a, b, c) printf("table fwd<%d,%d,%d>\n", a, b, c);
int main()
{
    HB_GROUP_KERNELS(G) HB_PERSIST_KERNELS(P) HB_DENSE_KERNELS(D) HB_FWD_KERNELS(F)
    for (int model = 1; model <= 6; model++)
    for (int nf = 2; nf <= (model == 6 ? 8 : 2); nf++)
    for (int P : {64, 128, 256, 512}) for (int Lv = 0; Lv <= 6; Lv++) for (int D = 1; D <= 8; D++) {
        if ((Lv + 1) * D - 1 > plan_band_limit(P, Lv, D)) continue; // (what hb_pipeline_geometry lets through)
        for (int bits = 0; bits < 16; bits++) {
            const bool cert = bits & 8, ca = bits & 4, ea = bits & 2, lg = bits & 1;
            const hb_sweep_plan p = plan_sweep(hb_sweep_shape{model, nf, P, Lv, D, std::max((Lv + 1) * D - 1, Lv), cert, ca, ea, lg, true});
            printf("%d %d %d %d %d %d %d %d %d | ", model, nf, P, Lv, D, cert, ca, ea, lg);
            if (!p.ok) { puts("unsupported"); continue; }
            if (p.chain == HB_CHAIN_GROUP) printf("group<%d,%d,%d,%d,%d> ", p.ct[0], p.ct[1], p.ct[2], p.ct[3], p.ct[4]);
            else if (p.chain == HB_CHAIN_PERSIST) printf("persist<%d,%d> ", p.ct[0], p.ct[1]);
            else printf("dense<%d> ", p.ct[0]);
            if (p.fwd[0]) printf("fwd<%d,%d,%d> ", p.fwd[0], p.fwd[1], p.fwd[2]); else printf("- ");
            printf("warm=%d/%d warm_r=%d/%d/%d fcorr=%d\n", p.warm, p.warm_ahead, p.warm_r, p.warm_r_ahead, p.warm_r_Lb, (int)p.fcorr);
        }
    }
}
"""


def test_every_sweep_plan_equals_the_recorded_dispatch_and_names_a_built_kernel(tmp_path):
    """plan_sweep (hibayes_amd/csrc/hb_plan.hpp: plain C++, compiled here with g++) decides which chain kernel a sweep of the persistent pipeline
    runs and what runs beside it. Every input of the domain — model 1..6 (n_fold 2..8 for BayesR), panel 64..512, every geometry the band limit
    lets through, certificate, the two "alone" switches, short / long range — against tests/golden/sweep_plan_table.json, which was recorded from
    the dispatch as it stood inside enqueue_sweep_pipeline before it became this function. And both ways between the plans and the lists of
    instantiations hb_kernels.hip builds its launch tables from (HB_*_KERNELS, the same header): a plan names only listed kernels, and every
    listed kernel is some input's plan."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "plan.cpp", tmp_path / "plan"
    src.write_text(_PLAN_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(root, "hibayes_amd", "csrc"), str(src), "-o", str(exe)])
    listed, got = set(), {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        if line.startswith("table "):
            listed.add(line[6:])
        else:
            k, v = line.split(" | ")
            got[tuple(int(x) for x in k.split())] = v
    assert len(listed) == 13 + 8 + 2 + 6
    table = json.load(open(os.path.join(root, "tests", "golden", "sweep_plan_table.json")))
    want = {}
    for key, gi in table["rows"].items():
        for Lv, row in enumerate(table["grids"][gi]):
            for D, ch in enumerate(row, start=1):
                if ch != ".":
                    model, nf, P, cert, ca, ea, lg = (int(x) for x in key.split())
                    want[(model, nf, P, Lv, D, cert, ca, ea, lg)] = "unsupported" if ch == "!" else table["outcomes"][ch]
    assert len(want) == 29568 and sum(v == "unsupported" for v in want.values()) == 364
    assert set(got) == set(want), "the domains differ (plan_band_limit?)"
    wrong = ["%s: %s, recorded %s" % (k, got[k], want[k]) for k in sorted(want) if got[k] != want[k]]
    assert not wrong, "%d plans differ from the record (model n_fold P Lv D cert chain_alone env_alone long_range), the first:\n%s" % (len(wrong), "\n".join(wrong[:20]))
    named = set()
    for v in got.values():
        if v != "unsupported":
            named.update(x for x in v.split()[:2] if x != "-")
    assert named <= listed, "plans name kernels that are in no launch table: %s" % sorted(named - listed)
    assert listed <= named, "listed kernels that no input of the domain runs: %s" % sorted(listed - named)


_RUNPLAN_PROGRAM = r"""
#include "hb_runplan.hpp"
#include <cmath>
#include <cstdio>
static const int MODEL_NF[12][2] = {{1, 2}, {2, 2}, {3, 2}, {4, 2}, {5, 2}, {6, 2}, {6, 3}, {6, 4}, {6, 5}, {6, 6}, {6, 7}, {6, 8}};
static const int ON_REGIMES[4][4] = {{3, 2, 2, 7}, {4, 2, 3, 7}, {3, 2, 2, 8}, {6, 4, 2, 2}}; // model, n_fold, Lv, D
static hb_regime on_regime(const int o[4]) { return plan_regime(o[0], o[1], 512, true, false, hb_geometry{1, o[2], o[3], 0, 0}, 27, false); }

// not in the record: every default geometry of an own context is one plan_sweep has kernels for, and the hysteresis holds between its thresholds
static void cross_properties()
{
    for (auto &mn : MODEL_NF) for (int P : {64, 128, 256, 512}) for (int row = 0; row < 2; row++) for (int wlv = 2; wlv <= 3; wlv++)
    for (int noad = 0; noad < 2; noad++) for (int conc = 0; conc < 2; conc++) for (int cert = 0; cert < 2; cert++) for (int lg = 0; lg < 2; lg++) {
        const hb_geometry a = plan_default_geometry(mn[0], mn[1], P, row, wlv, noad), g = plan_geometry(conc, a.pipeline, P, a.Lv, a.D);
        printf("sweep %d %d %d %d %d %d %d %d %d | %d\n", mn[0], mn[1], P, row, wlv, noad, conc, cert, lg,
               (int)plan_sweep(hb_sweep_shape{mn[0], mn[1], P, g.Lv, g.D, g.L, cert != 0, false, false, lg != 0, true}).ok);
    }
    for (auto &o : ON_REGIMES) {
        const hb_regime r = on_regime(o);
        for (int cur = 0; cur < 2; cur++) for (int k = 0; k <= 1000; k++) {
            const double pp = r.to_wide + (r.to_narrow - r.to_wide) * k / 1000.0;
            if (regime_next(r, cur, pp) != cur) printf("moved %d %d %d %d %d %.17g | 1\n", o[0], o[1], o[2], o[3], cur, pp);
        }
        printf("held %d %d %d %d | %d\n", o[0], o[1], o[2], o[3], (int)r.on);
    }
}

int main()
{
    for (int m : {100, 128, 255, 256, 300, 1023, 1024, 4095, 4096, 4608, 500000}) for (int moves = 0; moves < 2; moves++) for (int asked : {0, 64, 128, 256, 512})
        printf("panel %d %d %d | %d\n", m, moves, asked, plan_panel(m, moves, asked));
    for (int conc = 0; conc < 2; conc++) for (int pl = 0; pl < 2; pl++) for (int P : {64, 128, 256, 512})
    for (int Lv : {-1, 0, 1, 2, 3, 4, 5, 6, 9}) for (int D : {0, 1, 2, 3, 4, 5, 6, 7, 8, 12}) {
        const hb_geometry g = plan_geometry(conc, pl, P, Lv, D);
        printf("geometry %d %d %d %d %d | %d %d %d %d %d\n", conc, pl, P, Lv, D, g.pipeline, g.Lv, g.D, g.L, g.NB);
    }
    // the geometry of a context of the run's own: what it asks for, and what the context makes of it
    for (auto &mn : MODEL_NF) for (int P : {64, 128, 256, 512}) for (int row = 0; row < 2; row++) for (int wlv = 2; wlv <= 3; wlv++)
    for (int noad = 0; noad < 2; noad++) for (int conc = 0; conc < 2; conc++) {
        const hb_geometry a = plan_default_geometry(mn[0], mn[1], P, row, wlv, noad), g = plan_geometry(conc, a.pipeline, P, a.Lv, a.D);
        printf("default %d %d %d %d %d %d %d | %d %d %d -> %d %d %d %d %d\n", mn[0], mn[1], P, row, wlv, noad, conc, a.pipeline, a.Lv, a.D, g.pipeline, g.Lv, g.D, g.L, g.NB);
    }
    static const int CODES[3][2] = {{0, 3}, {-1, 2}, {0, 4}};
    static const long long SIZES[2][2] = {{4608, 512}, {500224, 50176}}; // m_pad, ld
    for (int bits : {0, 2, 8}) for (int own = 0; own < 2; own++) for (int row = 0; row < 2; row++) for (int precise = 1; precise <= 2; precise++)
    for (int noauto = 0; noauto < 2; noauto++) for (int pl = 0; pl < 2; pl++) for (auto &cd : CODES) for (int mem = 0; mem < 4; mem++)
    for (int P : {64, 128, 256, 512}) for (auto &mn : MODEL_NF) for (int wlv = 2; wlv <= 3; wlv++) for (auto &sz : SIZES) {
        // memory above band + packed + 2 GiB: the band is 7 * (wide_lv + 1) blocks for BayesB / C, 6 for BayesR
        const unsigned long long blocks = (mn[0] == 3 || mn[0] == 4) ? 7 * (wlv + 1) : 6;
        const unsigned long long bound = blocks * sz[0] * P * 4 + (unsigned long long)((sz[1] + 511) / 512 * 128) * sz[0] + (2ull << 30);
        const unsigned long long fr = mem == 0 ? 0 : mem == 1 ? bound : mem == 2 ? bound + 1 : (200ull << 30);
        printf("layout %d %d %d %d %d %d %d %d %d %d %d %d %d %lld | %d\n", bits, own, row, precise, noauto, pl, cd[0], cd[1], mem, P, mn[0], mn[1], wlv, sz[0],
               plan_layout(bits, own, row, precise, mn[0], mn[1], P, pl, cd[0], cd[1], noauto, (size_t)fr, (int)sz[0], (int64_t)sz[1], wlv));
    }
    for (auto &mn : MODEL_NF) for (int P : {64, 128, 256, 512}) for (int own = 0; own < 2; own++) for (int adp = 0; adp < 2; adp++)
    for (int noad = 0; noad < 2; noad++) for (int Lg : {0, 2, 4, 5, 19, 20, 27}) for (int pl = 0; pl < 2; pl++) for (int Lv = 0; Lv <= 6; Lv++) for (int D = 1; D <= 8; D++) {
        const hb_regime r = plan_regime(mn[0], mn[1], P, own, adp, hb_geometry{pl, Lv, D, 0, 0}, Lg, noad);
        printf("regime %d %d %d %d %d %d %d %d %d %d | ", mn[0], mn[1], P, own, adp, noad, Lg, pl, Lv, D);
        if (!r.on) { puts("off"); continue; }
        printf("wide %d %d narrow %d %d thresholds %.17g %.17g\n", r.Lv[0], r.D[0], r.Lv[1], r.D[1], r.to_wide, r.to_narrow);
    }
    // the hysteresis of each regime, at, beside and between its thresholds
    for (auto &o : ON_REGIMES) {
        const hb_regime r = on_regime(o);
        if (!r.on) continue;
        for (int cur = 0; cur < 2; cur++)
            for (int k = 0; k < 9; k++) { // moves per panel: 0, then below, at and above to_wide, half way, below, at and above to_narrow, then 1e6
                const double pp[9] = {0.0, std::nextafter(r.to_wide, 0.0), r.to_wide, std::nextafter(r.to_wide, 1e9), 0.5 * (r.to_wide + r.to_narrow),
                                      std::nextafter(r.to_narrow, 0.0), r.to_narrow, std::nextafter(r.to_narrow, 1e9), 1e6};
                printf("next %d %d %d %d %d %d | %d\n", o[0], o[1], o[2], o[3], cur, k, regime_next(r, cur, pp[k]));
            }
    }
    cross_properties();
}
"""


def test_every_run_plan_equals_the_recorded_decisions(tmp_path):
    """hb_runplan.hpp (plain C++, compiled here with g++) decides the configuration a run gives plan_sweep: the panel, the geometry a context
    normalises a request to, the geometry a run asks for on a context of its own, the resident layout, and whether and between which geometries
    the run follows the regime. Every stage over its domain against tests/golden/run_plan_table.json, which was recorded from the decision lines
    as they stood inside hb_run::setup, hb_run::step, hb_ctx_create and hb_pipeline_geometry before they became these functions. A few rows are
    asserted literally as well, read off that code: they guard the recording itself. Two properties across the stages: every default geometry,
    as a context normalises it, is one plan_sweep has kernels for, and the hysteresis changes nothing between its two thresholds."""
    import subprocess
    from run_plan_record import recorded_run_plan
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "runplan.cpp", tmp_path / "runplan"
    src.write_text(_RUNPLAN_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(root, "hibayes_amd", "csrc"), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        k, v = line.split(" | ")
        stage, key = k.split(" ", 1)
        got.setdefault(stage, {})[key] = v
    want = recorded_run_plan()
    assert {k: len(v) for k, v in want.items()} == {"panel": 110, "geometry": 1440, "default": 768, "layout": 221184, "regime": 301056, "next": 72}
    assert set(got) == set(want) | {"sweep", "held"}, "stages: %s" % sorted(got)  # (a "moved" row is a hysteresis that moved between its thresholds)
    for stage, rows in want.items():
        assert list(got[stage]) == list(rows), "the domains differ: %s" % stage
        wrong = ["%s: %s, recorded %s" % (k, got[stage][k], w) for k, w in rows.items() if got[stage][k] != w]
        assert not wrong, "%d rows of '%s' differ from the record, the first:\n%s" % (len(wrong), stage, "\n".join(wrong[:20]))
    assert len(got["sweep"]) == 3072 and set(got["sweep"].values()) == {"1"}, [k for k, v in got["sweep"].items() if v != "1"][:20]
    assert got["held"] == {"3 2 2 7": "1", "4 2 3 7": "1", "3 2 2 8": "1", "6 4 2 2": "1"}

    # ---- the literal rows ----
    def default(model, nf, P, row=0, wlv=2, noad=0, conc=1):  # -> (asked, the context's (pipeline, Lv, D), its band)
        asked, ctx = got["default"]["%d %d %d %d %d %d %d" % (model, nf, P, row, wlv, noad, conc)].split(" -> ")
        g = tuple(int(x) for x in ctx.split())
        return tuple(int(x) for x in asked.split()), g[:3], g[3]

    def regime(model, nf, P, own, adp, noad, Lg, pl, Lv, D):
        return got["regime"]["%d %d %d %d %d %d %d %d %d %d" % (model, nf, P, own, adp, noad, Lg, pl, Lv, D)]

    for model in (3, 4):  # BayesB / C on a context of the run's own
        assert default(model, 2, 512) == ((1, 2, 7), (1, 2, 7), 20) and default(model, 2, 512, wlv=3) == ((1, 3, 7), (1, 3, 7), 27)
        assert default(model, 2, 256, wlv=3)[1] == (1, 2, 7)
        assert all(default(model, 2, P, conc=0)[1] == (0, 2, 1) for P in (64, 128, 256, 512))  # (with wide_lv = 3: (0, 3, 1))
    for model in (1, 2, 5):  # BayesRR / A / L
        for m, P, geo in ((4096, 512, (1, 2, 2)), (500000, 512, (1, 2, 2)), (128, 128, (1, 2, 1)), (255, 128, (1, 2, 1)), (1024, 128, (1, 2, 1)), (4095, 128, (1, 2, 1))):
            assert int(got["panel"]["%d 1 0" % m]) == P and default(model, 2, P)[1] == geo, (model, m)
    for nf in (2, 3, 4):  # BayesR with up to four classes at panel 512
        assert default(6, nf, 512)[1] == (1, 2, 2) and regime(6, nf, 512, 1, 0, 0, 5, 1, 2, 2) == "wide 2 2 narrow 2 1 thresholds 22 27"
        assert default(6, nf, 512, noad=1)[1] == (1, 2, 1) and {regime(6, nf, 512, 1, 0, 1, 27, 1, 2, D) for D in (1, 2)} == {"off"}
    assert default(6, 5, 512)[1] == (1, 2, 1) and {regime(6, 5, 512, 1, 1, 0, 27, 1, 2, D) for D in (1, 2)} == {"off"}
    for model in (3, 4):  # BayesB / C: on only from (2 | 3, 7) or (2, 8) with a stored band of 20 panels or more
        on = {k: v for k, v in got["regime"].items() if k.startswith("%d 2 " % model) and v != "off"}
        assert len(on) == 4 * 3 * 2 * 2 * 3 and all(v == "wide %s narrow 2 2 thresholds 3.2000000000000002 4" % k[-3:] for k, v in on.items())
        for k in on:
            _, _, _, own, adp, _, Lg, pl, Lv, D = (int(x) for x in k.split())
            assert (own or adp) and Lg >= 20 and pl == 1 and (Lv, D) in ((2, 7), (3, 7), (2, 8)), k
    for k, v in got["default"].items():  # row mode
        if k.split()[3] == "1":
            assert v == "0 0 1 -> 0 0 1 0 1", k
    assert {v for k, v in got["layout"].items() if k.startswith("0 1 1 ")} == {"8"}
    for k, v in got["layout"].items():  # the automatic layout
        bits, own, row, precise, noauto, pl, xmin, xmax, mem, P, model, nf, _, _ = (int(x) for x in k.split())
        if bits == 0:
            assert (v == "2") == (own == 1 and row == 0 and precise == 2 and P == 512 and pl == 1 and noauto == 0 and (xmin, xmax) == (0, 3)
                                  and mem >= 2 and (model in (3, 4) or (model == 6 and nf <= 4))), k
        else:
            assert (v == "2") == (bits == 2 and own == 1), k


_REPLAYPLAN_PROGRAM = r"""
#include "hb_runplan.hpp"
#include <cstdio>

static void put(const hb_replay_step &d)
{
    printf("%d %d %d | %d %d %d %d\n", (int)d.replay, (int)d.to_per_panel, d.timeout_ms, d.state.aborts, d.state.win_start, d.state.win_count, d.state.slow_timeout);
}

// a run with recovery on, no HB_TIMEOUT_MS and a context bound of 3000 ms: sweeps[k] = {iteration, aborts of that sweep}
static void sequence(const char *name, const int (*sweeps)[2], int count)
{
    hb_replay_state st{};
    for (int k = 0; k < count; k++) {
        const int iter = sweeps[k][0];
        int bound = replay_first_wait_ms(true, false, 3000, st);
        bool fell_back = false;
        for (int attempt = 0; attempt < sweeps[k][1]; attempt++) {
            const hb_replay_step d = replay_after_abort(true, attempt, fell_back, iter, bound, st);
            printf("seq %s %d %d %d | %d -> ", name, k, iter, attempt, bound);
            put(d);
            if (!d.replay) break;
            fell_back = fell_back || d.to_per_panel;
            bound = d.timeout_ms;
            st = d.state;
        }
    }
}

int main()
{
    for (int on = 0; on < 2; on++) for (int pl = 0; pl < 2; pl++) for (int row = 0; row < 2; row++)
        printf("on %d %d %d | %d\n", on, pl, row, (int)replay_enabled(on, pl, row));
    for (int rec = 0; rec < 2; rec++) for (int env = 0; env < 2; env++) for (int ctx : {100, 3000, 5000}) for (int slow : {0, 400, 1600, 3000}) {
        hb_replay_state st{2, 40, 1, slow};
        const int first = replay_first_wait_ms(rec, env, ctx, st);
        printf("first %d %d %d %d | %d\n", rec, env, ctx, slow, first);
        // an abort at iteration 50 of a run whose window opened at 40 with one abort: the bound in force is the sweep's first one at attempt 0, a replay's after it
        for (int fb = 0; fb < 2; fb++) for (int attempt = 0; attempt <= 4; attempt++) {
            printf("after %d %d %d %d %d %d | ", rec, env, fb, attempt, ctx, slow);
            put(replay_after_abort(rec, attempt, fb, 50, attempt == 0 ? first : (first > 3000 ? first : 3000), st));
        }
    }
    static const int escalates[7][2] = {{0, 1}, {10, 1}, {20, 1}, {30, 1}, {40, 1}, {50, 1}, {60, 1}};       // 100 -> 400 -> 1600 -> 3000, capped
    static const int reset_at_65[5][2] = {{0, 1}, {30, 1}, {65, 1}, {66, 1}, {67, 1}};                       // more than 64 iterations: a new window
    static const int holds_at_64[3][2] = {{0, 1}, {30, 1}, {64, 1}};                                         // 64 iterations: the same window
    static const int two_a_window[6][2] = {{0, 1}, {5, 1}, {200, 1}, {205, 1}, {400, 1}, {464, 1}};          // never three: no escalation
    static const int one_sweep[2][2] = {{7, 4}, {8, 1}};                                                     // the fourth failure of a sweep ends the run
    static const int stays_raised[4][2] = {{0, 1}, {1, 1}, {2, 1}, {500, 2}};                                // a new window keeps the raised bound
    sequence("escalates", escalates, 7);
    sequence("reset_at_65", reset_at_65, 5);
    sequence("holds_at_64", holds_at_64, 3);
    sequence("two_a_window", two_a_window, 6);
    sequence("one_sweep", one_sweep, 2);
    sequence("stays_raised", stays_raised, 4);
}
"""


def test_every_replay_decision_equals_the_recorded_policy(tmp_path):
    """hb_runplan.hpp's "replaying an aborted sweep" (plain C++, compiled here with g++) decides what follows a sweep whose pipeline gave up waiting:
    whether recovery is on at all, the wait bound a sweep starts with, and after an abort whether to replay, whether to fall back to the per-panel
    kernels first, the replay's bound and what the run has learnt about the device. Against tests/golden/replay_plan_table.json, which was recorded
    from the statements as they stood inside hb_run::step() before they became these functions: every combination of recover, HB_TIMEOUT_MS given
    and fallen back, attempts 0-4, context bounds of 100, 3000 and 5000 ms, and runs of aborts by iteration number. The rows the policy is quoted
    by are asserted literally as well, read off that code: they guard the recording itself."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "replayplan.cpp", tmp_path / "replayplan"
    src.write_text(_REPLAYPLAN_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(root, "hibayes_amd", "csrc"), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        k, v = line.split(" | ", 1)
        stage, key = k.split(" ", 1)
        got.setdefault(stage, {})[key] = v
    want = json.load(open(os.path.join(root, "tests", "golden", "replay_plan_table.json")))
    assert {k: len(v) for k, v in want.items()} == {"on": 8, "first": 48, "after": 480, "seq": 31}
    assert set(got) == set(want)
    for stage, rows in want.items():
        assert list(got[stage]) == list(rows), "the domains differ: %s" % stage
        wrong = ["%s: %s, recorded %s" % (k, got[stage][k], w) for k, w in rows.items() if got[stage][k] != w]
        assert not wrong, "%d rows of '%s' differ from the record, the first:\n%s" % (len(wrong), stage, "\n".join(wrong[:20]))

    # ---- the literal rows ----
    assert [k for k, v in got["on"].items() if v == "1"] == ["1 1 0"]  # HB_RECOVER on, the persistent pipeline, individuals not sharded
    for ctx in (100, 3000, 5000):  # the first try waits 100 ms — unless HB_TIMEOUT_MS fixed the bound, the run learnt better, or nothing replays
        assert got["first"]["1 0 %d 0" % ctx] == "100" and got["first"]["1 0 %d 1600" % ctx] == "1600"
        assert {got["first"]["%d %d %d 400" % (rec, env, ctx)] for rec, env in ((0, 0), (0, 1), (1, 1))} == {str(ctx)}
    for k, v in got["after"].items():  # (the state before: 2 sweeps replayed, one abort in the window that iteration 40 opened; the abort is at 50)
        rec, env, fb, attempt, ctx, slow = (int(x) for x in k.split())
        first = max(100, slow) if rec and not env else ctx
        if not rec or attempt >= 3:  # the fourth failure of a sweep ends the run, and so does the first without recovery
            assert v == "0 0 %d | 2 40 1 %d" % (first if attempt == 0 else max(first, 3000), slow), k
        else:  # a replay waits 3 s or the bound in force; the second time-out of a sweep falls back, once
            assert v == "1 %d %d | 3 40 2 %d" % (attempt >= 1 and not fb, max(first, 3000), slow), k

    def slow_after(name):  # per sweep and attempt: (the bound the sweep started with or the replay had, slow_timeout afterwards)
        return [(int(v.split()[0]), int(v.split()[-1])) for k, v in got["seq"].items() if k.startswith(name + " ")]

    assert slow_after("escalates") == [(100, 0), (100, 0), (100, 400), (400, 1600), (1600, 3000), (3000, 3000), (3000, 3000)]
    assert slow_after("reset_at_65") == [(100, 0)] * 4 + [(100, 400)] and slow_after("holds_at_64") == [(100, 0), (100, 0), (100, 400)]
    assert {s for _, s in slow_after("two_a_window")} == {0}
    assert [v.split(" | ")[0] for k, v in got["seq"].items() if k.startswith("one_sweep 0 ")] == ["100 -> 1 0 3000", "3000 -> 1 1 3000", "3000 -> 1 0 3000", "3000 -> 0 0 3000"]
    assert got["seq"]["stays_raised 3 500 0"] == "400 -> 1 0 3000 | 4 500 1 400"


_MATVECPLAN_PROGRAM = r"""
#include "hb_matvecplan.hpp"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#define M(ct, g, sc) printf("table k_dotq2m<%d,%d,%d> %d\n", ct, g, sc, q2m_lds(ct, g));
#define Q(cpl, rs) printf("table k_dotq2<%d,%d> %d\n", cpl, rs, q2_lds(cpl, rs));
static const char *fake_name, *fake_val;
static const char *fake_getenv(const char *k) { return fake_name && !strcmp(k, fake_name) ? fake_val : nullptr; }

// one family's rows: its knobs (the key's prefix) over ld x ncols x num_cus x update rows x finalize rows
static void rows(const char *stage, const char *prefix, int layout, const hb_matvec_knobs &k)
{
    std::vector<int> widths;
    for (int w = 64; w <= 4096; w += 64)
        for (int P : {64, 128, 256, 512}) if (w % P == 0 && w / P <= 8) { widths.push_back(w); break; }
    for (long long ld : {256, 512, 768, 1024, 1280, 1536, 2048, 5120, 50176, 131072, 174080, 400384}) for (int ncols : widths) for (int cus : {32, 64, 256})
    for (int upd = 0; upd < (layout == 8 ? 3 : 2); upd++) for (int fin = 0; fin < 4; fin++) {
        const int nupd = upd == 0 ? 0 : (int)(ld / (upd == 2 ? 64 : 256)), fin_ncols = fin == 0 ? 0 : fin == 1 ? ncols / 2 : fin == 2 ? ncols : 2 * ncols;
        const int nfin = (fin_ncols + 63) / 64;
        const hb_matvec_plan p = plan_matvec(hb_matvec_shape{layout, ld, 128 * ((ld + 511) / 512), ncols, nupd, nfin, upd == 2, cus}, k);
        char name[64];
        if (p.family == HB_MV_DOTQ2M) snprintf(name, sizeof name, "k_dotq2m<%d,%d,%d>", p.arg[0], p.arg[1], p.arg[2]);
        else if (p.family == HB_MV_DOTQ2) snprintf(name, sizeof name, "k_dotq2<%d,%d>", p.arg[0], p.arg[1]);
        else snprintf(name, sizeof name, p.family == HB_MV_DOTQ2R ? "k_dotq2r" : "k_dotq");
        // what the record holds | what the arithmetic invariants read
        printf("%s %s %lld %d %d %d %d | %s %d %d %d %d %d | %d %d %d %d\n", stage, prefix, ld, ncols, cus, upd, fin, name, p.nstages, p.ncg, p.lds, p.NS,
               p.ncg ? p.tiles / p.ncg : -1, p.tiles, p.blocks, nupd, nfin);
    }
}

int main()
{
    HB_DOTQ2M_KERNELS(M) HB_DOTQ2_KERNELS(Q)
    printf("table k_dotq %d\ntable k_dotq2r 0\nneed %d\n", HBQ_LDS, 512 * 4 + 512 * 8); // (need: the update rows' move lists, HBU_ROWS_LDS of hb_update.hpp)
    char pre[64];
    for (int t : {256, 768, 2000}) { hb_matvec_knobs k; k.dotq_tiles = t; snprintf(pre, sizeof pre, "%d", t); rows("dotq", pre, 8, k); }
    for (int cpl : {1, 2}) for (int rs : {128, 256, 512}) for (int t : {400, 1600, 2000}) {
        hb_matvec_knobs k; k.kind = 0; k.dotq2_cpl = cpl; k.dotq2_rs = rs; k.dotq2_tiles = t; k.dotq2_tiles_set = true;
        snprintf(pre, sizeof pre, "%d %d %d", cpl, rs, t); rows("dotq2", pre, 2, k);
    }
    for (int nc : {4, 8, 12, 16, 32}) { hb_matvec_knobs k; k.kind = 1; k.nc = nc; snprintf(pre, sizeof pre, "%d", nc); rows("dotq2r", pre, 2, k); }
    for (int sc : {0, 1}) for (int g : {0, 1, 2, 3}) for (int ct : {4, 8, 16}) for (int t : {0, 400, 800, 1600}) { // (t == 0: HB_DOTQ2_TILES not given)
        hb_matvec_knobs k; k.q2m_sc = sc; k.q2m_g = g; k.q2m_ct = ct;
        if (t) k.dotq2_tiles = t, k.dotq2_tiles_set = true;
        snprintf(pre, sizeof pre, "%d %d %d %d", sc, g, ct, t); rows("dotq2m", pre, 2, k);
    }
    for (const char *n : {"HB_DOTQ_TILES", "HB_DOTQ2_TILES", "HB_DOTQ2_KIND", "HB_DOTQ2_CPL", "HB_DOTQ2_RS", "HB_DOTQ2_NC", "HB_Q2M_CT", "HB_Q2M_G", "HB_Q2M_SC"})
    for (const char *r : {"unset", "0", "1", "2", "3", "4", "7", "8", "12", "15", "16", "17", "33", "128", "256", "400", "512", "2000", "-1", "x", "empty"}) {
        fake_name = strcmp(r, "unset") ? n : nullptr;
        fake_val = strcmp(r, "empty") ? r : "";
        const hb_matvec_knobs k = matvec_knobs_from_env(fake_getenv);
        printf("knobs %s %s | %d %d %d %d %d %d %d %d %d %d\n", n, r, k.dotq_tiles, k.dotq2_tiles, (int)k.dotq2_tiles_set, k.kind, k.dotq2_cpl, k.dotq2_rs, k.nc, k.q2m_ct, k.q2m_g, k.q2m_sc);
    }
}
"""


def test_every_matvec_plan_equals_the_recorded_launch_and_names_a_built_kernel(tmp_path):
    """plan_matvec (hibayes_amd/csrc/hb_matvecplan.hpp: plain C++, compiled here with g++) decides what one launch of the fixed-point panel mat-vec is:
    kernel and template arguments, stages per tile, tiles, blocks, LDS. Every input of the domain — twelve column lengths from one stage to beyond
    the int32 bound, every width of one to eight panels, riders, 32 / 64 / 256 compute units, and per kernel family every value its knobs' clamps
    can produce — against tests/golden/matvec_plan_table.json, which was recorded from the decision as it stood inside launch_dotq2 / launch_dotq
    and hb_ctx_create before it became this header. Both ways between the plans and the lists hb_kernels.hip builds its launch table from; the
    LDS of a plan is its listed kernel's and holds the update rows' move lists; the arithmetic every launch relies on; and the rows DESIGN.md
    quotes, literally (they guard the recording itself)."""
    import subprocess
    from run_plan_record import recorded_matvec_plan
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "matvecplan.cpp", tmp_path / "matvecplan"
    src.write_text(_MATVECPLAN_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(root, "hibayes_amd", "csrc"), str(src), "-o", str(exe)])
    listed, got, extra, need = {}, {}, {}, None
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        if line.startswith("table "):
            listed[line.split()[1]] = int(line.split()[2])
        elif line.startswith("need "):
            need = int(line.split()[1])
        else:
            k, v = line.split(" | ", 1)
            stage, key = k.split(" ", 1)
            v, _, more = v.partition(" | ")
            got.setdefault(stage, {})[key] = v
            if more:
                extra[(stage, key)] = tuple(int(x) for x in more.split())
    assert len(listed) == 14 + 5 + 2 and min(v for k, v in listed.items() if k != "k_dotq2r") >= need == 6144
    want = recorded_matvec_plan()
    assert {k: len(v) for k, v in want.items()} == {"dotq": 25920, "dotq2": 103680, "dotq2r": 28800, "dotq2m": 552960, "knobs": 189}
    assert set(got) == set(want)
    for stage, rows in want.items():
        assert list(got[stage]) == list(rows), "the domains differ: %s" % stage
        wrong = ["%s: %s, recorded %s" % (k, got[stage][k], w) for k, w in rows.items() if got[stage][k] != w]
        assert not wrong, "%d rows of '%s' differ from the record, the first:\n%s" % (len(wrong), stage, "\n".join(wrong[:20]))
    named = set()
    for (stage, key), (tiles, blocks, nupd, nfin) in extra.items():
        kernel, nstages, ncg, lds, NS, trows = got[stage][key].split()
        nstages, ncg, lds, NS, trows = int(nstages), int(ncg), int(lds), int(NS), int(trows)
        named.add(kernel)
        assert tiles == ncg * trows and blocks == nupd + nfin + tiles, (stage, key)
        if kernel == "k_dotq2r":  # (NS is its columns per tile: every row block a tile row)
            assert trows == nstages and NS * ncg == int(key.split()[-4]) and lds == 0, (stage, key)
            continue
        assert NS * trows >= nstages and (NS - 1) * trows < nstages + trows, (stage, key)
        if kernel == "k_dotq":
            assert NS <= 1023, (stage, key)  # (NS * 128 rows * 128 * 128 < 2^31: every int8 code, -128 included)
            assert lds == (24832 if key.split()[-2] == "2" else listed[kernel]), (stage, key)  # (HBU_LDS where the dense update rows ride)
        else:
            stage_rows = 512 if kernel.startswith("k_dotq2m<4,0") or kernel.startswith("k_dotq2m<4,3") else 256 if kernel[7] == "m" else int(kernel[10:-1])
            assert NS * stage_rows <= 131072 and lds == listed[kernel], (stage, key)
    assert named <= set(listed), "plans name kernels that are in no launch table: %s" % sorted(named - set(listed))
    assert set(listed) <= named, "listed kernels that no input of the domain runs: %s" % sorted(set(listed) - named)

    # ---- the literal rows: the knobs' defaults, 256 compute units, update rows ld / 256 and finalize rows ncols / 64 where they ride ----
    def plan(stage, knobs, ld, ncols, riders):
        key = "%s %d %d 256 %s" % (knobs, ld, ncols, "1 2" if riders else "0 0")
        kernel, nstages, ncg, _, NS, _ = got[stage][key].split()
        return (kernel, int(nstages), int(NS), int(ncg)) + extra[(stage, key)][:2]

    assert plan("dotq2m", "1 0 4 0", 50176, 3584, True) == ("k_dotq2m<4,0,1>", 98, 9, 56, 616, 868)
    assert plan("dotq2m", "1 0 4 0", 50176, 3584, False)[:5] == ("k_dotq2m<4,0,1>", 98, 7, 56, 784)
    assert plan("dotq2m", "1 0 4 0", 50176, 1024, True) == ("k_dotq2m<4,0,1>", 98, 5, 16, 320, 532)
    assert plan("dotq2", "1 256 1600", 50176, 3584, True)[:5] == ("k_dotq2<1,256>", 196, 7, 56, 1568)
    assert plan("dotq2r", "16", 50176, 3584, True)[:5] == ("k_dotq2r", 13, 16, 224, 2912)
    assert plan("dotq", "768", 50176, 3584, True) == ("k_dotq", 392, 28, 56, 784, 1036)
    assert plan("dotq2m", "1 0 4 0", 768, 512, False) == ("k_dotq2m<4,1,1>", 3, 3, 8, 8, 8)      # (768 is no multiple of 512: G falls back to 1)
    assert plan("dotq2m", "1 0 4 0", 400384, 3584, True)[:5] == ("k_dotq2m<4,0,1>", 782, 196, 56, 224)  # (196 stages of 512: the int32 floor)


_TRI_TILE_PROGRAM = r"""
#include "hb_mma.hpp"
#include <cstdio>
static long long seen = 0, wrong = 0;
static void check(long long x)
{
    int bi = -1, bj = -1;
    tri_tile(x, &bi, &bj);
    seen++;
    if (!(0 <= bj && bj <= bi && (long long)bi * (bi + 1) / 2 + bj == x) && wrong++ < 20) printf("wrong %lld -> (%d, %d)\n", x, bi, bj);
}
int main()
{
    for (int T : {1, 2, 3, 157})
        for (long long x = 0; x < (long long)T * (T + 1) / 2; x++) check(x);
    for (long long c : {46340LL, 2000000LL})
        for (long long bi = c - 64; bi <= c + 64; bi++)
            for (long long d = -2; d <= 2; d++) check(bi * (bi + 1) / 2 + d);
    printf("checked %lld wrong %lld\n", seen, wrong);
}
"""


def test_tri_tile_decodes_every_block_index_of_a_lower_triangle(tmp_path):
    """tri_tile (hibayes_amd/csrc/hb_mma.hpp, __host__ __device__: the host half of the very text k_grm_tile, k_eig_trail and k_eig_gram run, compiled
    here by hipcc for the host alone) turns a linear block index into the tile (bi, bj), bj <= bi, of a lower triangle. Every index of the
    triangles of 1, 2, 3 and 157 tiles a side, and the two indices either side of every boundary bi (bi + 1) / 2 for the 129 bi around 46 340 —
    where bi (bi + 1) passes 2^31 — and around 2 000 000, where the fp64 square root that seeds the search can be one off: 0 <= bj <= bi and
    bi (bi + 1) / 2 + bj == index."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "tri_tile.cpp", tmp_path / "tri_tile"
    src.write_text(_TRI_TILE_PROGRAM)
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-std=c++17", "-Wall", "-Werror", "-I",
                           os.path.join(root, "hibayes_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().splitlines()
    assert out == ["checked %d wrong 0" % (1 + 3 + 6 + 157 * 158 // 2 + 2 * 129 * 5)], "\n".join(out)
