#!/usr/bin/env python
"""Time of BSLMM's dense side on the device (hb_grm.hip): the polygenic block of one iteration — three passes over the n x n fp64
eigenvector matrix — with its bytes per second beside the streaming-read rate bench.py quotes as roofline.measured_copy_GBps
(Context.time_stream_read) and hb_cg's dense pass (profiles/cg_timing.txt), and the build of the relationship matrix with its int8
multiply-accumulate rate. Needs a GPU and torch (the random K is made on the device: timing needs no eigen-decomposition).

    python tools/bslmm_time.py [--n 20000] [--m 100000] [--out profiles/bslmm_timing.txt]

The block's time is wall time over `--steps` enqueued iterations between two synchronisations: what the sampler pays per iteration,
launch gaps included, not a kernel time. Bytes per iteration are what the algorithm must read: K three times (3 n^2 8) plus the
partial sums of K w written and re-read and the n-long vectors. MACs of the build: n^2 m / 2 (one triangle)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hibayes_amd as H  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if H.lib().hb_device_count() < 1:
        raise SystemExit("bslmm_time.py: no HIP device visible")
    import torch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("command: python tools/bslmm_time.py " + " ".join(sys.argv[1:]))
    n, m = a.n, a.m
    with H.Context(20000, 20000) as ctx:                                            # bench.py's ceiling: a plain streaming read of 400 MB
        ctx.generate(5)
        ms, nb = ctx.time_stream_read(reps=3)
    copy = nb / (ms * 1e-3) / 1e9
    say("streaming read of %.0f MB of resident genotypes (bench.py's roofline.measured_copy_GBps): %.0f GB/s" % (nb / 1e6, copy))

    # ---- the polygenic block ----
    with H.Context(n, 64) as c:
        c.generate(6)
        ld = n + (n & 1)
        g = torch.Generator(device="cuda").manual_seed(7)
        K = torch.randn((n, ld), dtype=torch.float64, device="cuda", generator=g) / np.sqrt(n)   # any K with positive Kval will do
        Kval = np.random.default_rng(8).uniform(0.05, 3.0, n)
        c.poly_setup(Kval, K, on_device=True)
        rng = np.random.default_rng(9)
        c.set_residual(rng.normal(size=n), np.zeros(n))
        c.poly_step(1.0, 0.5, 1, 0, float(n), 0.1)                                  # warm-up: code objects
        c.poly_state()
        per = []
        for rep in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for it in range(a.steps):
                c.poly_step(1.0, -1.0, 1, 1 + rep * a.steps + it, float(n), 0.1)
            _, vb, q, flag = c.poly_state()
            per.append((time.perf_counter() - t) / a.steps)
        rowblocks = ((n + 1) // 2 + 255) // 256                                     # hb_ctx_poly_setup's choice of column chunks
        cpc = max(64, -(-n // max(1, 2048 // rowblocks)))
        nchunk = -(-n // cpc)
        by = 3 * n * ld * 8 + 2 * nchunk * ld * 8 + 16 * n * 8
        best = min(per)
        say("polygenic block, n = %d (K %.2f GB, %d column chunks in K w): %.3f ms per iteration (three runs of %d: %s), %.1f MB -> %.0f GB/s, "
            "%.3f of the streaming-read rate; per pass over K %.3f ms" % (n, n * ld * 8 / 1e9, nchunk, 1e3 * best, a.steps,
                                                                         " ".join("%.3f" % (1e3 * p) for p in per), by / 1e6, by / best / 1e9,
                                                                         by / best / 1e9 / copy, 1e3 * best / 3))
        say("(hb_cg's dense pass on the same card and size: profiles/cg_timing.txt; vb = %.6g, q = %.6g, flag = %s after the last step)" % (vb, q, flag))
        del K

    # ---- the relationship matrix ----
    with H.Context(n, m) as c:
        c.generate(10)
        c.marker_stats()
        L = H.lib()
        import ctypes as C
        per = []
        for rep in range(3):
            dev = C.c_void_p()
            t = time.perf_counter()
            H._lib.check(L.hb_grm_build(c.h, 0.0, 0, None, C.byref(dev)))
            per.append(time.perf_counter() - t)
            L.hb_grm_free(dev)
        best = min(per)
        macs = 0.5 * n * n * m
        say("make_grm, n = %d, m = %d (result left on the device): %.3f s (three builds: %s) -> %.1f T int8 MAC/s over one triangle" %
            (n, m, best, " ".join("%.3f" % p for p in per), macs / best / 1e12))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
