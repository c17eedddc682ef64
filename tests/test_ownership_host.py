"""Every device and pinned allocation has an owner (hibayes_amd/csrc/hb_bufs.hpp), checked without a device: the header alone against a stand-in
for <hip/hip_runtime.h> whose allocations count and can be refused; the sources, which call the runtime's allocation functions nowhere else; and
the built library's count of what it holds (hb_debug_live_buffers)."""
import glob
import os
import re
import subprocess
import sys

import hibayes_amd as H
from hibayes_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hibayes_amd", "csrc")
CALLS = ("hipMalloc", "hipExtMallocWithFlags", "hipHostMalloc", "hipFree", "hipHostFree")

# the stand-in: the handful of types, the five allocation and free calls, hipMemsetAsync, hipGetErrorString and hipGetLastError. Every allocation
# is recorded with its kind, its size and how often it was freed; refuse_at = k makes the k-th allocation (from 1) fail as the runtime's does, with
# the caller's pointer left as it was. Fresh memory is filled with 0xAB, so that a buffer that reads zero was zeroed.
STAND_IN = r"""
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
typedef struct stub_stream *hipStream_t;
enum { hipDeviceMallocFinegrained = 1, hipDeviceMallocUncached = 3 };
struct stub_alloc { void *p; size_t bytes; int kind; int freed; int wrong_free; }; // kind: 0 hipMalloc, 1 uncached, 2 fine-grained, 3 pinned
inline std::vector<stub_alloc> stub_allocs;
inline int stub_seen = 0, stub_refuse_at = 0, stub_unknown_frees = 0, stub_last_error_reads = 0;
inline hipError_t stub_new(void **p, size_t bytes, int kind)
{
    if (++stub_seen == stub_refuse_at) return hipErrorOutOfMemory;
    *p = malloc(bytes);
    memset(*p, 0xAB, bytes);
    stub_allocs.push_back({*p, bytes, kind, 0, 0});
    return hipSuccess;
}
inline hipError_t stub_delete(void *p, bool pinned)
{
    for (stub_alloc &a : stub_allocs)
        if (a.p == p && !a.freed) {
            a.freed++;
            if ((a.kind == 3) != pinned) a.wrong_free++;
            free(p);
            return hipSuccess;
        }
    for (stub_alloc &a : stub_allocs)
        if (a.p == p) { a.freed++; return hipSuccess; } // a second free of the same buffer: counted, not carried out
    stub_unknown_frees++;
    return hipSuccess;
}
inline hipError_t hipMalloc(void **p, size_t bytes) { return stub_new(p, bytes, 0); }
inline hipError_t hipExtMallocWithFlags(void **p, size_t bytes, unsigned flags) { return stub_new(p, bytes, flags == hipDeviceMallocUncached ? 1 : 2); }
inline hipError_t hipHostMalloc(void **p, size_t bytes, unsigned = 0) { return stub_new(p, bytes, 3); }
inline hipError_t hipFree(void *p) { return stub_delete(p, false); }
inline hipError_t hipHostFree(void *p) { return stub_delete(p, true); }
inline hipError_t hipMemsetAsync(void *p, int v, size_t bytes, hipStream_t) { memset(p, v, bytes); return hipSuccess; }
inline const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "out of memory"; }
inline hipError_t hipGetLastError() { stub_last_error_reads++; return hipSuccess; }
"""

PROGRAM = r"""
#include "hb_bufs.hpp"
#include <cstdio>
#include <cstring>

static std::string g_text;
static int g_failed = 0;
int hb_fail(int status, const std::string &msg) { g_text = msg; return status; }

#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) { printf("line %d (refuse_at %d): %s\n", __LINE__, stub_refuse_at, #cond); g_failed++; } \
    } while (0)

static int64_t live_n() { return hb_live_count.load(); }
static int64_t live_b() { return hb_live_bytes.load(); }
static void reset(int refuse_at)
{
    stub_allocs.clear();
    stub_seen = 0, stub_refuse_at = refuse_at, stub_unknown_frees = 0;
}
static bool all_zero(const void *p, size_t bytes)
{
    for (size_t i = 0; i < bytes; i++)
        if (static_cast<const unsigned char *>(p)[i]) return false;
    return true;
}
static void every_allocation_freed_once()
{
    for (const stub_alloc &a : stub_allocs) CHECK(a.freed == 1 && a.wrong_free == 0);
    CHECK(stub_unknown_frees == 0);
}

// get / zeroed / pin / hand-off / big in a row, as an entry point makes them: the first refusal ends it (HB_TRY). step k is allocation k.
static void sequence(int refuse_at, int handoff_kind)
{
    reset(refuse_at);
    const int64_t n0 = live_n(), b0 = live_b();
    int reached = 0;
    {
        hb_bufs m;
        double *a = reinterpret_cast<double *>(8), *e = reinterpret_cast<double *>(8), *c = reinterpret_cast<double *>(8);
        int *b = reinterpret_cast<int *>(8);
        unsigned *d = reinterpret_cast<unsigned *>(8);
        int64_t n = n0, by = b0;
        auto after = [&](int rc, const void *p, size_t bytes) { // the step that has just run
            reached++;
            if (reached == refuse_at) {
                CHECK(rc == HB_ERR_HIP && p == nullptr);
                CHECK(g_text.find("out of memory") != std::string::npos);
                return false;
            }
            n += 1, by += (int64_t)bytes;
            CHECK(rc == HB_OK && p != nullptr && p != reinterpret_cast<void *>(8));
            CHECK(live_n() == n && live_b() == by);
            return true;
        };
#define STEP(call, ptr, bytes)                  \
    {                                           \
        const int rc_ = (call);                 \
        if (!after(rc_, ptr, bytes)) break;     \
    }
        do {
            STEP(m.get(&a, 10), a, 80);
            STEP(m.zeroed(&b, 5, nullptr), b, 20);
            CHECK(all_zero(b, 20));
            STEP(m.pin(&c, 4), c, 32);
            STEP(m.handoff(&d, 8, nullptr), d, 32);
            CHECK(all_zero(d, 32) && stub_allocs.back().kind == handoff_kind);
            STEP(m.get(&a, 0), a, 8); // (a count of 0 is one element: never a null pointer that succeeded)
            g_text.clear();
            STEP(m.big(&e, (size_t)12500000, "hb_some_entry", "the " + hb_dims(300) + " matrix"), e, (size_t)100000000);
        } while (0);
        if (refuse_at == 6) { // the big allocator's text
            CHECK(g_text == "hb_some_entry: hipMalloc: out of memory \xe2\x80\x94 the 300 x 300 matrix needs 0.1 GB on the device");
        }
        CHECK(live_n() == n && live_b() == by); // (a refusal changes nothing)
        CHECK((int)stub_allocs.size() == (refuse_at ? refuse_at - 1 : 6));
    }
    every_allocation_freed_once();
    CHECK(live_n() == n0 && live_b() == b0);
}

static void drop_release_give()
{
    reset(0);
    const int64_t n0 = live_n(), b0 = live_b();
    double *kept = nullptr;
    {
        hb_bufs m, other;
        double *a = nullptr, *b = nullptr, *c = nullptr, *g = nullptr, *none = nullptr;
        CHECK(m.get(&a, 3) == HB_OK && m.get(&b, 5) == HB_OK && m.pin(&c, 7) == HB_OK && m.get(&kept, 11) == HB_OK && m.get(&g, 13) == HB_OK);
        CHECK(live_n() == n0 + 5 && live_b() == b0 + 8 * (3 + 5 + 7 + 11 + 13));
        m.drop(&a); // device
        CHECK(a == nullptr && stub_allocs[0].freed == 1 && live_n() == n0 + 4 && live_b() == b0 + 8 * (5 + 7 + 11 + 13));
        m.drop(&a); // (null: nothing)
        m.drop(&none);
        m.drop(&c); // pinned: the other free call
        CHECK(c == nullptr && stub_allocs[2].freed == 1 && stub_allocs[2].wrong_free == 0 && live_n() == n0 + 3);
        m.release(kept); // the caller's
        CHECK(live_n() == n0 + 3 && stub_allocs[3].freed == 0);
        m.give(other, g); // another owner's
        CHECK(live_n() == n0 + 3 && stub_allocs[4].freed == 0);
        m.clear();
        CHECK(stub_allocs[0].freed == 1 && stub_allocs[1].freed == 1 && stub_allocs[2].freed == 1 && stub_allocs[3].freed == 0 && stub_allocs[4].freed == 0);
        CHECK(live_n() == n0 + 2 && live_b() == b0 + 8 * (11 + 13));
        m.clear(); // (again: nothing left)
        CHECK(m.get(&b, 2) == HB_OK); // the owner goes on after a clear()
    }
    CHECK(stub_allocs[4].freed == 1 && stub_allocs[5].freed == 1 && stub_allocs[3].freed == 0);
    CHECK(live_n() == n0 + 1 && live_b() == b0 + 8 * 11);
    hb_free_released(kept);
    CHECK(stub_allocs[3].freed == 1 && live_n() == n0 && live_b() == b0);
    hb_free_released(kept); // (no longer known: left alone)
    hb_free_released(nullptr);
    {   // a buffer the caller can do without: refused quietly, taken like any other
        hb_bufs m;
        double *t = reinterpret_cast<double *>(8);
        g_text = "untouched";
        stub_refuse_at = stub_seen + 1;
        CHECK(!m.try_get(&t, 9) && t == nullptr && g_text == "untouched" && live_n() == n0 && live_b() == b0);
        CHECK(m.try_get(&t, 9) && t != nullptr && live_n() == n0 + 1 && live_b() == b0 + 72);
    }
    every_allocation_freed_once();
    CHECK(live_n() == n0 && live_b() == b0);
}

int main()
{
    const char *env = getenv("HB_HANDOFF_ALLOC");
    const int kind = env ? atoi(env) : 0;
    CHECK(hb_handoff_kind() == kind);
    for (int k = 0; k <= 6; k++) sequence(k, kind);
    drop_release_give();
    CHECK(live_n() == 0 && live_b() == 0);
    CHECK(stub_last_error_reads == 7); // every refusal was cleared from the runtime's last-error slot, nothing else was
    printf("%s\n", g_failed ? "FAILED" : "ok");
    return g_failed ? 1 : 0;
}
"""


def test_hb_bufs_alone_frees_everything_once_on_every_way_out(tmp_path):
    inc = tmp_path / "hip"
    inc.mkdir()
    (inc / "hip_runtime.h").write_text(STAND_IN)
    src, exe = tmp_path / "own.cpp", tmp_path / "own"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", str(tmp_path), "-I", CSRC, str(src), "-o", str(exe)])
    for kind in (None, "1", "2"):  # the hand-off memory's kind is read once per process
        env = {k: v for k, v in os.environ.items() if k != "HB_HANDOFF_ALLOC"}
        if kind:
            env["HB_HANDOFF_ALLOC"] = kind
        r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_only_hb_bufs_calls_the_allocation_functions():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
    assert len(files) > 40
    found = {c: [] for c in CALLS}
    for f in files:
        text = open(f).read()
        for c in CALLS:
            if re.search(r"\b%s\b" % c, text):
                found[c].append(os.path.basename(f))
    for c in CALLS:
        assert found[c] == ["hb_bufs.hpp"], (c, found[c])
    for name, gone in (("hb_ctx.hip", r"#define\s+TRY\b"), ("hb_grm.hip", r"\bPOLY_TRY\b"), ("hb_epsl.hip", r"\bEPSL_TRY\b"), ("hb_chol.hip", r"\bchol_mem\b")):
        assert not re.search(gone, open(os.path.join(CSRC, name)).read()), (name, gone)
    internal = open(os.path.join(CSRC, "hb_internal.hpp")).read()
    assert '#include "hb_bufs.hpp"' in internal and "struct hb_bufs" not in internal and "#define HB_HIP" not in internal


# a fresh process: nothing is held when the library is loaded, and nothing after calls that fail for want of a device (those of the
# "without a device" tests of test_eig_host.py, test_stedc_host.py, test_chol_host.py and test_ldmat_host.py). Where a device is visible those
# calls would run: a small inverse and a refusal stand in for them there.
_FRESH = r"""
import ctypes as C
import numpy as np
import hibayes_amd as H
from hibayes_amd import eig as HE
from hibayes_amd.engine import live_buffers

L = H.lib()
assert live_buffers() == (0, 0), live_buffers()
nb, by = C.c_int64(7), C.c_int64(7)
assert L.hb_debug_live_buffers(C.byref(nb), None) == 0 and L.hb_debug_live_buffers(None, C.byref(by)) == 0 and L.hb_debug_live_buffers(None, None) == 0
assert (nb.value, by.value) == (0, 0)

def refused(f, *a, **k):
    try:
        f(*a, **k)
    except H.HibayesError as e:
        assert e.status == 2 and "no HIP device available" in str(e), str(e)
    else:
        raise AssertionError("not refused")
    assert live_buffers() == (0, 0), live_buffers()

if L.hb_device_count() < 1:
    G = np.cov(np.random.default_rng(1).normal(size=(17, 40)))
    d, e = np.arange(1.0, 18.0), np.full(16, 0.5)
    T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
    refused(H.eigh, G)
    refused(H.eigh, T, tridiagonal="device")
    refused(H.make_grm, np.ones((5, 7), dtype=np.int8), 0.01, eigen=True, eigen_solver="device", verbose=False)
    refused(H.make_grm, np.ones((5, 7), dtype=np.int8), 0.01, eigen=True, eigen_solver="device", tridiagonal="device", verbose=False)
    refused(HE.tridiagonal_eigh_device, d, e)
    refused(HE.tridiagonal_eigh_device, np.ones(1), None)
    refused(H.spd_inverse, np.eye(3))
    refused(H.ldmat, (np.arange(35).reshape(5, 7) % 3).astype(np.int8))
    buf, info = np.eye(4, order="F"), C.c_int32()
    for rc in (L.hb_spd_inverse(buf.ctypes.data, 4, 4, 0, 0.0, C.byref(info)), L.hb_chol_factor(buf.ctypes.data, 4, 4, 0, 0.0, C.byref(info)),
               L.hb_chol_invert_factor(buf.ctypes.data, 4, 4, 0)):
        assert rc == 2 and live_buffers() == (0, 0)
else:
    assert np.array_equal(H.spd_inverse(np.diag([1.0, 4.0, 0.25])), np.diag([1.0, 0.25, 4.0]))
    assert live_buffers() == (0, 0), live_buffers()
    buf, info = np.eye(4, order="F"), C.c_int32()
    assert L.hb_spd_inverse(buf.ctypes.data, 3, 4, 0, 0.0, C.byref(info)) == 1 and live_buffers() == (0, 0)
print("ok")
"""


def test_the_library_counts_what_it_holds_and_holds_nothing_when_loaded():
    lib = H.lib()
    hdr = open(os.path.join(ROOT, "include", "hibayes_gpu.h")).read()
    assert "hb_debug_live_buffers" in _lib.SYMBOLS and hasattr(lib, "hb_debug_live_buffers")
    assert re.search(r"\bint\s+hb_debug_live_buffers\s*\(\s*int64_t\s*\*\s*buffers\s*,\s*int64_t\s*\*\s*bytes\s*\)\s*;", hdr)
    assert lib.hb_abi_version() == 6
    from hibayes_amd.engine import live_buffers
    n, b = live_buffers()
    assert n >= 0 and b >= 0 and (n == 0) == (b == 0)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _FRESH], env=env, capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
