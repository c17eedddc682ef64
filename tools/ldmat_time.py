"""Time of ldmat() on the device beside the Gram build of the same context.
   python tools/ldmat_time.py [n] [m] [dense|sparse|gram ...]  ->  one JSON line per build
Genotypes are generated on the device (hb_ctx_generate_genotype). dense = the genome-wide matrix, sparse = chisq 5; each line
splits the build into BigStat / strips (cross-products and epilogue, k_ld_strip) / compaction / device-to-host copies and gives
k_ld_strip's int8 MAC/s (m * m * ld per build: the padded rows are multiplied too); gram = hb_ctx_build_gram's band of the same
context, the MAC/s of k_gram_tiled — the same tile loop (hb_mma.hpp's mma_i8_staged) without the fp64 epilogue and the strip writes."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hibayes_amd as H  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
m = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
what = sys.argv[3:] or ["dense", "sparse", "gram"]

with H.Context(n, m) as c:
    c.generate(20240901, mono_every=97)
    ld = c.ld
    for w in what:
        if w == "gram":
            s = c.build_gram()
            P, L = c.panel, c.pipeline()[3]
            npan = -(-m // P)
            blocks = sum(min(p, L) + 1 for p in range(npan))
            macs = blocks * P * P * ld
            print(json.dumps({"build": "gram", "n": n, "m": m, "panel": P, "band_blocks": blocks, "seconds": round(s, 4),
                              "int8_mac_per_s": macs / s}), flush=True)
            continue
        for rep in range(2):                                   # the first build pays the kernels' load
            with c.ldmat(chisq=5.0 if w == "sparse" else None) as l:
                st = l.info()
        macs = float(m) * m * ld
        print(json.dumps({"build": w, "n": n, "m": m, "ld": ld, "strips": st["n_strips"], "nnz": st["nnz"], "device_copy": bool(st["on_device"]),
                          "seconds": round(st["seconds"], 4), "stats_seconds": round(st["stats_seconds"], 4),
                          "strip_seconds": round(st["strip_seconds"], 4), "compact_seconds": round(st["compact_seconds"], 4),
                          "transfer_seconds": round(st["transfer_seconds"], 4), "k_ld_strip_int8_mac_per_s": macs / st["strip_seconds"]}), flush=True)
