#!/usr/bin/env python
"""Time of the sweep on the fp64 resident layout (real-valued genotypes, genotype_bits = 64; hb_real.hip): sweeps per second of BayesCpi and
BayesRR, the time per panel of its three kernels (k_dot_real, k_chain<K1, double>, k_update_real), the mat-vec's bytes per second beside the
streaming-read rate of the same buffer (Context.time_stream_read: the measured ceiling, not the data sheet's), the Gram set-up, and the CPU
oracle's time per sweep on the same data. Needs a GPU.

    python tools/real_timing.py [--n 50000] [--m 50000] [--iters 20] [--oracle-iters 2] [--out profiles/real_timing.txt]

The genotypes are generated on the device as 0/1/2 codes and converted there to fp64 columns (hb_ctx_set_layout(c, 64, 0)): the kernels' time
does not depend on the values, and a 20 GB host matrix need not exist. Sweeps per second are hb_bayes_run's own loop time over `--iters`
iterations on that context; the per-kernel times come from one sweep run in the HIP-event timing mode (set_profiling(1): the same kernels,
serialised on one stream)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hibayes_amd as H  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--m", type=int, default=50000)
    ap.add_argument("--panel", type=int, default=0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--oracle-iters", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if H.lib().hb_device_count() < 1:
        raise SystemExit("real_timing.py: no HIP device visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("command: python tools/real_timing.py " + " ".join(sys.argv[1:]))
    n, m = a.n, a.m
    rng = np.random.default_rng(11)
    y = rng.normal(0, 1, n)
    with H.Context(n, m, panel=a.panel) as c:
        c.generate(12)
        X8 = c.download() if a.oracle_iters > 0 else None
        t = time.perf_counter()
        c.set_layout(64)
        say("n = %d, m = %d, panel %d: %.2f GB of fp64 columns (converted on the device in %.2f s)" % (n, m, c.panel, c.ld * 8 * m / 1e9, time.perf_counter() - t))
        ms, nb = c.time_stream_read(reps=3)
        copy = nb / (ms * 1e-3) / 1e9
        say("streaming read of the same buffer (%.2f GB): %.2f ms -> %.0f GB/s" % (nb / 1e9, ms, copy))
        t = time.perf_counter()
        c.marker_stats()
        say("k_stats_real (two passes): %.3f s" % (time.perf_counter() - t))
        gs = c.build_gram()
        npan = -(-m // c.panel)
        say("Gram set-up (k_gram_real, %d diagonal blocks of %d x %d on the fp64 matrix cores): %.3f s" % (npan, c.panel, c.panel, gs))
        for model, Pi in (("BayesCpi", [0.95, 0.05]), ("BayesRR", [0.95, 0.05])):
            r = H.Bayes(y, None, model, Pi, ctx=c, niter=a.iters, nburn=a.iters // 2, thin=1, verbose=False, store_alpha=False)
            tm = r["timing"]
            sps = tm["iters_done"] / tm["loop_seconds"]
            say("%s: %.2f sweeps/s (%d iterations in %.3f s, %.1f moves per sweep, resident_bits %d)" %
                (model, sps, tm["iters_done"], tm["loop_seconds"], tm["mean_events"], tm["resident_bits"]))
            # one more sweep in the timing mode: the same kernels, serialised, with HIP events around each
            c.set_profiling(1)
            r2 = H.Bayes(y, None, model, Pi, ctx=c, niter=3, nburn=1, thin=1, verbose=False, store_alpha=False, g_init=r["last"]["g"], warm=r["last"]["warm"])
            T = c.last_timing()
            c.set_profiling(0)
            by = c.ld * 8 * npan * c.panel
            say("%s, one sweep serialised: %.2f ms = mat-vec %.2f + chain %.2f + update %.2f + other %.2f; per panel: mat-vec %.1f us, chain %.1f us, "
                "update %.1f us; mat-vec %.0f GB/s = %.2f of the streaming-read rate; %d dependent launches (3 per panel)" %
                (model, T["total_ms"], T["dot_ms"], T["chain_ms"], T["update_ms"], T["other_ms"], 1e3 * T["dot_ms"] / npan, 1e3 * T["chain_ms"] / npan,
                 1e3 * T["update_ms"] / npan, by / (T["dot_ms"] * 1e-3) / 1e9, by / (T["dot_ms"] * 1e-3) / 1e9 / copy, 3 * npan))
            del r2
    if a.oracle_iters > 0:
        from oracle import oracle as O
        thr = min(16, os.cpu_count() or 1)
        for model, Pi in (("BayesCpi", [0.95, 0.05]), ("BayesRR", [0.95, 0.05])):
            t = time.perf_counter()
            ref = O.bayes(y, X8, model, Pi, niter=a.oracle_iters, nburn=0, thin=1, threads=thr, rng=O.RNG_PHILOX)
            say("oracle (CPU, %d threads, the same genotypes as int8), %s: %.2f s per sweep (%d sweeps; its own loop time %.2f s, %.1f s with set-up)" %
                (thr, model, ref["loop_seconds"] / max(1, ref["iters_done"]), ref["iters_done"], ref["loop_seconds"], time.perf_counter() - t))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
