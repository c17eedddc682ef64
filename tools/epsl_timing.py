#!/usr/bin/env python
"""Time of the single-step model's epsilon block on the device (hb_epsl.hip) on synthetic pedigrees: per iteration,
the block alone, and an iteration of Bayes() with and without it; the schedule's levels, launches and stored entries; the same Gibbs pass
as a sequential single-thread C++ loop (compiled here with g++, the same arithmetic: no contraction); and the host imputation of ssbrm()'s
set-up (one sparse LU factor of A^-1_nn, solves in column chunks) on the same pedigrees.

    python tools/epsl_timing.py [--q 100000 1000000] [--shapes 5x4 20x4 20x40 80x4] [--out profiles/epsl_timing.txt]
    python tools/epsl_timing.py --impute-only ...        (no GPU needed: the imputation's part alone)
    python tools/epsl_timing.py --impute-device --q 20000 100000 1000000 --out profiles/impute_timing.txt
                                                         (the device imputation, hb_impute.hip; up to --host-max beside the host's)

A pedigree of `generations x family`: founders, then generations of equal size in which every sire of the previous generation has `family`
offspring with dams drawn at random from it; the last-but-one tenth of the youngest generation is genotyped, a tenth of the rest of it has a
record. Generations deepen the dependency graph (levels), the family size widens the sires' columns.
The block's time is wall time over `--steps` enqueued steps between two synchronisations: what the sampler pays per iteration, launch gaps
included, not a kernel time."""
import argparse
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hibayes_amd as H  # noqa: E402
from hibayes_amd.ssbayes import epsl_plan  # noqa: E402

CPP = r"""
#include <cmath>
#include <cstdint>
extern "C" void epsl_pass(int q, const int64_t *indptr, const int32_t *indices, const double *data, const double *diag, const double *zz,
                          const double *b, double *x, const double *z, double lam, double vare)
{
    for (int i = 0; i < q; i++) {
        double s = 0.0;
        for (int64_t k = indptr[i]; k < indptr[i + 1]; k++) s = s + data[k] * x[indices[k]];
        const double aii = zz[i] + lam * diag[i];
        const double Ax = zz[i] * x[i] + lam * s;
        x[i] = ((b[i] - Ax) / aii + x[i]) + std::sqrt(vare / aii) * z[i];
    }
}
"""


def pedigree(total, generations, family, seed, selfing=True):
    """(s, d): 1-based parents, parents first; `generations` generations after the founders, every one of total / (generations + 1).
    selfing=False draws the dams from the individuals that are not sires: no offspring then has one individual as both parents. (With the
    default about one offspring in a thousand has, make_Ainv() gives that parent the reference's 1.5 where Henderson's rule has 2, and
    A^-1_nn is no longer positive definite — the Gibbs pass does not mind, conjugate gradients do.)"""
    rng = np.random.default_rng(seed)
    size = max(2 * family, total // (generations + 1))
    s, d = [np.zeros(size, dtype=np.int64)], [np.zeros(size, dtype=np.int64)]
    first = 0
    for _ in range(generations):
        prev = np.arange(first, first + size) + 1
        nsire = max(1, size // family)
        sires = rng.choice(prev, nsire, replace=False)
        s.append(np.repeat(sires, family)[:size] if nsire * family >= size else np.resize(np.repeat(sires, family), size))
        d.append(rng.choice(prev if selfing else np.setdiff1d(prev, sires), size))
        first += size
    return np.concatenate(s), np.concatenate(d), size


def impute_device_leg(a, say):
    """The device imputation on the generated pedigrees (without selfing: see pedigree()): set-up (validation and upload) and solve, per block
    width and column count; up to --host-max individuals also the host's route — the LU factor and its solve — on the same systems and columns.
    Times are host clocks around calls that end in a synchronisation; the product kernel alone is timed by the library with device events
    (HB_IMPUTE_PROFILE), its bytes are counted from the shapes: a row of W doubles per stored entry, Ap written, the matrix read."""
    from hibayes_amd.impute import ImputeSystem
    from scipy.sparse.linalg import splu
    os.environ["HB_IMPUTE_PROFILE"] = "1"
    if H.lib().hb_device_count() < 1:
        raise SystemExit("epsl_timing.py --impute-device: no HIP device visible")
    for total in a.q:
        for shape in a.shapes:
            gens, fam = [int(v) for v in shape.split("x")]
            s, d, size = pedigree(total, gens, fam, 1, selfing=False)
            N = s.size
            geno = np.arange(N - size, N - size + size // 10)
            is_g = np.zeros(N, dtype=bool)
            is_g[geno] = True
            Ai = H.make_Ainv(s, d, one_parent="henderson").tocsr()
            n_indx = np.flatnonzero(~is_g)
            Ann = Ai[n_indx][:, n_indx].tocsc()
            Ann.sort_indices()
            Ang = Ai[n_indx][:, geno].tocsr()
            Ang.sort_indices()
            q = Ann.shape[0]
            say("pedigree %d x %d of %d: q_e = %d, %d genotyped, %d stored entries in A^-1_nn, %d in A^-1_ng; tol = %g"
                % (gens, fam, N, q, geno.size, Ann.nnz, Ang.nnz, a.impute_tol))
            lu = None
            if q <= a.host_max:
                t0 = time.perf_counter()
                lu = splu(Ann, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
                say("    host: LU factor %.2f s (%d + %d stored entries in L + U)" % (time.perf_counter() - t0, lu.L.nnz, lu.U.nnz))
            for cols in a.impute_cols_list:
                M = np.asfortranarray(np.random.default_rng(2).integers(0, 3, size=(geno.size, cols)).astype(np.float64))
                t0 = time.perf_counter()
                with ImputeSystem(Ann, Ang) as S:
                    t_setup = time.perf_counter() - t0
                    S.solve(M[:, :1], a.impute_tol, 20000)  # (the first launches load the code object)
                    runs = []
                    for rep in range(a.impute_reps):
                        x, st = S.solve(M, a.impute_tol, 20000)
                        runs.append(st["seconds"])
                best = min(runs)
                say("    device, %d columns: set-up %.3f s, solve %.4f s (%s) = %.3f ms per column; W = %d, %d block(s), %d iterations, %d looks, p %s "
                    "the cache rule; largest true residual %.3g" % (cols, t_setup, best, " ".join("%.4f" % r for r in runs), 1e3 * best / cols, st["width"],
                                                                    st["blocks"], st["iterations"], st["looks"], "within" if st["cached"] else "beyond",
                                                                    st["max_residual"]))
                say("        = %.1f us per iteration of a block (three launches); the product kernel alone %.1f us per launch, %.1f MB counted: %.2f TB/s"
                    % (1e6 * best / max(1, st["blocks"] * st["iterations"]), 1e6 * st["product_seconds"], st["product_bytes"] / 1e6,
                       st["product_bytes"] / max(st["product_seconds"], 1e-12) / 1e12))
                if lu is not None:
                    t0 = time.perf_counter()
                    xh = lu.solve(-(Ang @ M))
                    t_solve = time.perf_counter() - t0
                    say("        host solve of the same columns %.3f s = %.2f ms per column; largest |device - host| %.3g (largest |host| %.3g)"
                        % (t_solve, 1e3 * t_solve / cols, float(np.max(np.abs(x - xh))), float(np.max(np.abs(xh)))))
                    del xh
                del x, M
            del lu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--q", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--shapes", nargs="+", default=["5x4", "20x4", "20x40", "80x4"], help="generations x family size")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--m", type=int, default=2000, help="markers of the Bayes() runs")
    ap.add_argument("--ng", type=int, default=2000, help="genotyped records of the Bayes() runs")
    ap.add_argument("--impute-cols", type=int, default=64)
    ap.add_argument("--impute-only", action="store_true")
    ap.add_argument("--no-impute", action="store_true")
    ap.add_argument("--impute-device", action="store_true", help="the device imputation's leg alone")
    ap.add_argument("--impute-cols-list", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--impute-tol", type=float, default=1e-12)
    ap.add_argument("--impute-reps", type=int, default=2)
    ap.add_argument("--host-max", type=int, default=25000, help="largest q_e at which the host's factor is run beside the device")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)

    say("command: python tools/epsl_timing.py " + " ".join(sys.argv[1:]))
    if a.impute_device:
        impute_device_leg(a, say)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    gpu = not a.impute_only
    if gpu and H.lib().hb_device_count() < 1:
        raise SystemExit("epsl_timing.py: no HIP device visible (--impute-only needs none)")
    seq = None
    if gpu:
        d = tempfile.mkdtemp()
        with open(os.path.join(d, "pass.cpp"), "w") as f:
            f.write(CPP)
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(d, "pass.cpp"), "-o", os.path.join(d, "pass.so")])
        seq = C.CDLL(os.path.join(d, "pass.so")).epsl_pass
        seq.argtypes = [C.c_int] + [C.c_void_p] * 8 + [C.c_double, C.c_double]
        seq.restype = None
        import atexit
        atexit.register(shutil.rmtree, d, True)
    for total in a.q:
        for shape in a.shapes:
            gens, fam = [int(v) for v in shape.split("x")]
            s, d, size = pedigree(total, gens, fam, 1)
            N = s.size
            young = np.arange(N - size, N)
            geno = young[: size // 10]
            is_g = np.zeros(N, dtype=bool)
            is_g[geno] = True
            t0 = time.perf_counter()
            Ai = H.make_Ainv(s, d, one_parent="henderson").tocsr()
            n_indx = np.flatnonzero(~is_g)
            Ann = Ai[n_indx][:, n_indx].tocsc()
            Ann.sort_indices()
            t_ainv = time.perf_counter() - t0
            q = Ann.shape[0]
            pl = epsl_plan(Ann)
            kinds = [int(k) for k, _, _ in pl["launches"]]
            say("pedigree %d x %d of %d (q_e = %d, %d genotyped): A^-1 in %.2f s; %d stored entries, longest column %d, %d levels, %d launches "
                "(%d single-workgroup, %d wide)" % (gens, fam, N, q, geno.size, t_ainv, Ann.nnz, pl["max_col"], pl["levels"], len(kinds), kinds.count(0),
                                                     kinds.count(1)))
            if not a.no_impute:
                from scipy.sparse.linalg import splu
                Ang = Ai[n_indx][:, geno].tocsr()
                M = np.random.default_rng(2).integers(0, 3, size=(geno.size, a.impute_cols)).astype(np.float64)
                t0 = time.perf_counter()
                lu = splu(Ann, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
                t_lu = time.perf_counter() - t0
                t0 = time.perf_counter()
                Mn = lu.solve(-(Ang @ M))
                t_solve = time.perf_counter() - t0
                say("    host imputation: LU factor %.2f s (%d + %d stored entries in L + U), solve of %d marker columns %.2f s = %.1f ms per column"
                    % (t_lu, lu.L.nnz, lu.U.nnz, a.impute_cols, t_solve, 1e3 * t_solve / a.impute_cols))
                del lu, Mn
            if not gpu:
                continue
            rng = np.random.default_rng(3)
            rec_ind = np.flatnonzero(~is_g[N - size:])                      # the youngest generation's non-genotyped: a tenth has a record
            rec_ind = rec_ind[: max(1, rec_ind.size // 10)]
            pos = np.cumsum(~is_g) - 1                                      # position among the non-genotyped
            index1 = pos[N - size + rec_ind] + 1
            ne = index1.size
            n = a.ng + ne
            yJ = np.concatenate([np.full(a.ng, -1.0), rng.uniform(-1.0, 0.0, ne)])
            y = rng.normal(size=n)
            X = rng.integers(0, 3, size=(n, a.m)).astype(np.int8)
            G = (Ann.indptr, Ann.indices, Ann.data)
            # ---- the block alone ----
            with H.Context(n, 8) as c:
                c.upload(np.zeros((n, 8), dtype=np.int8))
                c.epsl_setup(yJ, G, index1)
                c.set_residual(y, np.zeros(n))
                c.epsl_step(1.0, 0.5, 1, 0, 0.1, float(q), 0.1)
                c.epsl_state()
                per = []
                for rep in range(3):
                    t0 = time.perf_counter()
                    for it in range(a.steps):
                        c.epsl_step(1.0, -1.0, 1, 1 + rep * a.steps + it, 0.1, float(q), 0.1)
                    x, veps, qv, J = c.epsl_state()
                    per.append((time.perf_counter() - t0) / a.steps)
                dbg = c.epsl_debug()
            # ---- the same pass, sequential on one host thread ----
            diag = Ann.diagonal()
            zz = np.bincount(index1 - 1, minlength=q).astype(np.float64)
            xs, z = np.zeros(q), rng.normal(size=q)
            indptr, indices = np.ascontiguousarray(Ann.indptr, dtype=np.int64), np.ascontiguousarray(Ann.indices, dtype=np.int32)
            hp = []
            for rep in range(3):
                t0 = time.perf_counter()
                seq(q, indptr.ctypes.data, indices.ctypes.data, Ann.data.ctypes.data, diag.ctypes.data, zz.ctypes.data, dbg["b"].ctypes.data, xs.ctypes.data,
                    z.ctypes.data, 2.0, 1.0)
                hp.append(time.perf_counter() - t0)
            say("    block alone: %.3f ms per iteration (three runs of %d: %s); veps %.4g. Sequential C++ pass (the rows only, one thread): %.3f ms (%s)"
                % (1e3 * min(per), a.steps, " ".join("%.3f" % (1e3 * p) for p in per), veps, 1e3 * min(hp), " ".join("%.3f" % (1e3 * p) for p in hp)))
            # ---- an iteration with and without it ----
            kw = dict(niter=40, nburn=20, thin=5, verbose=False, store_alpha=False, seed=5)
            r0 = H.Bayes(y, X, "BayesCpi", [0.95, 0.05], **kw)
            r1 = H.Bayes(y, X, "BayesCpi", [0.95, 0.05], epsl_y_J=yJ, epsl_Gi=G, epsl_index=index1, store_epsilon=False, **kw)
            say("    Bayes() BayesCpi, n = %d (%d + %d records), m = %d, %d bits resident: %.3f ms per iteration without the block, %.3f ms with it"
                % (n, a.ng, ne, a.m, r1["timing"]["resident_bits"], 1e3 * r0["timing"]["loop_seconds"] / 40, 1e3 * r1["timing"]["loop_seconds"] / 40))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
