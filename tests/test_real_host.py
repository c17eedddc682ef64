"""The fp64 resident layout (real-valued genotypes, genotype_bits = 64) as far as a machine without a GPU can see it: the library exports its
entry points under the unchanged ABI number, the header declares them to a C compiler, and the compiler's resource report of its kernels
(hibayes_amd/csrc/hb_real.res.txt and the fp64 instantiations of k_chain in hb_kernels.res.txt, both kept by the Makefile) shows no scratch."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hibayes_amd", "csrc")
NEW_SYMBOLS = ("hb_ctx_upload_genotype_real", "hb_ctx_download_genotype_real", "hb_ctx_download_gram_real")


def test_library_exports_the_real_entry_points_under_abi_6():
    import hibayes_amd as H
    from hibayes_amd._lib import LIB_PATH, SYMBOLS
    raw = ctypes.CDLL(LIB_PATH)
    for s in NEW_SYMBOLS:
        assert hasattr(raw, s), "%s is not exported" % s
        assert s in SYMBOLS
    assert H.lib().hb_abi_version() == 6


def test_header_declares_the_real_entry_points_to_a_c_caller(tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('#include "hibayes_gpu.h"\n'
                   "int up(hb_ctx *c, const double *X, double *Y, double *G) {\n"
                   "    return hb_ctx_upload_genotype_real(c, X, 8) + hb_ctx_download_genotype_real(c, Y, 8) + hb_ctx_download_gram_real(c, 0, G); }\n"
                   "int main(void) { return hb_abi_version() == HB_ABI_VERSION ? 0 : 1; }\n")
    exe = str(tmp_path / "caller")
    libdir = os.path.join(ROOT, "hibayes_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", libdir, "-lhibayes_gpu", "-Wl,-rpath," + libdir, "-o", exe])
    assert subprocess.run([exe]).returncode == 0


def _report(path):
    assert os.path.exists(path), "%s is missing: the Makefile writes it when it compiles the unit" % path
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
    return rows


def test_real_kernels_are_built_without_scratch():
    rows = _report(os.path.join(CSRC, "hb_real.res.txt"))
    for name in ("k_real_check", "k_i8_to_real", "k_stats_real", "k_dot_real", "k_gram_real", "k_gram_real_finish", "k_update_real",
                 "k_xalpha_real", "k_xmat_real"):
        found = [k for k in rows if re.match(r"_Z\d+%s[A-Z]" % name, k)]
        assert found, "kernel missing from the report: %s" % name
        for k in found:
            assert rows[k].get("ScratchSize", 0) == 0 and rows[k].get("VGPRsSpill", 0) == 0 and rows[k].get("SGPRsSpill", 0) == 0, (k, rows[k])
    # the chain on an fp64 Gram block: k_chain<K1, double>, K1 = 1, 3, 7 (hb_kernels.hip)
    rows = _report(os.path.join(CSRC, "hb_kernels.res.txt"))
    for k1 in (1, 3, 7):
        k = "_Z7k_chainILi%dEdEvPK11hb_sweep_in10chain_viewii" % k1
        assert k in rows, "kernel missing from the report: k_chain<%d, double>" % k1
        assert rows[k].get("ScratchSize", 0) == 0 and rows[k].get("VGPRsSpill", 0) == 0, (k, rows[k])
