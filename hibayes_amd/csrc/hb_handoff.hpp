// hb_handoff.hpp — the hand-off words of the persistent pipeline: flag block, agent-scope loads / write-through stores, bounded waits, the abort log (the wave and block sums are hb_wave.hpp's).
// Part of the one translation unit hb_kernels.hip (the kernels share device globals and the views defined before them);
// included there in this order, not compiled on its own.
#pragma once
#include "hb_wave.hpp"

// ---- device-side flags of the persistent pipeline ----
// Every shared word is accessed with relaxed agent-scope atomics (sc1); payloads are written with 4/8-byte
// agent-scope atomic stores (write-through) and drained with s_waitcnt vmcnt(0) before the flag moves, so no
// release fence is needed; consumers read the payload with agent-scope atomic loads (sc1), so no acquire
// fence either (cdna_hip_programming.md §6 Guideline 16, forms R1 / "sc1 both sides").
#define HB_FLAG_CHAIN_DONE 0
#define HB_FLAG_ABORT 1
#define HB_FLAG_XCC 2               /* 1 + the XCD the chain workgroup runs on (k_warm) */
#define HB_NFLAGS 72                /* words in the flag block that every sweep clears */
// How long a wait inside the pipeline may last before it gives up and aborts the sweep, in ticks of wall_clock64() (100 MHz). A device
// global, set per sweep from hb_ctx.timeout_ms (hbk_set_timeout): 100 ms by default — a healthy hand-off takes microseconds, the
// device's own occasional pauses ~1 ms (§9.0), and an aborted sweep is replayed by hb_run_step, so giving up early is cheap; the
// replay of a sweep runs with 3 s, and a run that aborts repeatedly (a shared or profiled GPU) raises its own default.
__device__ unsigned long long hb_timeout_ticks = 10000000ull;
#define HB_TIMEOUT_TICKS hb_timeout_ticks
// Abort log (diagnostics of a pipeline time-out, read by fetch_acc in hb_ctx.hip): whoever leaves a wait because the sweep is
// being aborted appends one record of 8 words — what it was waiting for, whether the time-out was its own, the clock, the value
// it last saw. flags[HB_FLAG_LOGN] counts the records, they start at flags + HB_LOG_BASE (the flag block has 4096 words).
#define HB_FLAG_LOGN 64
#define HB_LOG_BASE 128
#define HB_LOG_CAP 480
#define HB_LOG_CHAIN_DOT 1    /* k_chain_dense: a = marker index into dsum[], b = panel */
#define HB_LOG_CHAIN_FCORR 2  /* ... into fcorr[] */
#define HB_LOG_CHAIN_FC2 3    /* ... into fcorr2[] */
#define HB_LOG_FOLD_DD 4      /* k_fold_dense: a = index into dd[], b = target panel | step << 16 */
#define HB_LOG_UPD_DENSE 5    /* update_rows_dense: a = first panel of the group, b = block */
#define HB_LOG_WAIT_GE 6      /* wait_ge: a = word, b = value wanted */
#define HB_LOG_GROUP 7        /* k_chain_group / k_fwd / k_chain_persist: a = code, b = panel or group */

__device__ __forceinline__ unsigned ld_flag(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_flag(unsigned *p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ld_sc1(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ld_sc1(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// (write-through stores that the writer's L2 forwards; publishing with a no-return atomic exchange at the memory side instead was an
// A/B for the dense stall and changed nothing)
__device__ __forceinline__ void st_sc1(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_sc1(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __attribute__((noinline)) void hb_abort_log(unsigned *flags, unsigned kind, bool own, unsigned a, unsigned b, unsigned long long seen)
{
    const unsigned i = atomicAdd(flags + HB_FLAG_LOGN, 1u);
    if (i >= HB_LOG_CAP) return;
    unsigned *r = flags + HB_LOG_BASE + 8 * i;
    const unsigned long long now = wall_clock64();
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    r[0] = kind | (own ? 0x10000u : 0u) | ((xcc & 15u) << 20);
    r[1] = a;
    r[2] = b;
    r[3] = blockIdx.x;
    r[4] = (unsigned)now;
    r[5] = (unsigned)(now >> 32);
    r[6] = (unsigned)seen;
    r[7] = (unsigned)(seen >> 32);
}

// Polling pace: a waiter looks again after a short sleep. (Stretching the sleep of a long wait did not help the dense stall)
__device__ __forceinline__ void hb_poll_pause(int base)
{
    if (base <= 1) __builtin_amdgcn_s_sleep(1);
    else __builtin_amdgcn_s_sleep(8);
}

// A look that cannot be served a stale line. The hand-offs are polled with agent-scope (sc1) loads, which the XCD's L2 may serve. A
// returning agent-scope atomic (fetch-or with 0) is performed at the memory side, the one place all eight XCDs agree on: it returns what
// memory holds and leaves it unchanged. The waits of the pipeline do not look this way: the dense stall of round 3 — one write-through
// store of the chain workgroup in nobody's view for seconds after one of the device's ~1 ms pauses, profiles/r04_dense_stall_diagnostics.txt
// — is on the WRITER's side, and neither memory-side looks in every wait nor a write-back of the waiter's own L2 after a few hundred looks
// released it (11 sweeps in 16 000 still timed out, §9.0). hb_reduce.hpp and the re-look of hb_update.hpp read this way.
__device__ __forceinline__ double ld_fresh(const double *p)
{
    return __longlong_as_double((long long)__hip_atomic_fetch_or(reinterpret_cast<unsigned long long *>(const_cast<double *>(p)), 0ull,
                                                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ int ld_fresh(const int *p)
{
    return (int)__hip_atomic_fetch_or(reinterpret_cast<unsigned *>(const_cast<int *>(p)), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// (uniform) is this look of a wait a memory-side one? Settled: never. Two waits still ask — the take of k_chain_persist and the opening of
// k_chain_group — because hipcc allocates registers (persist) and schedules three instructions of the stamps build (group) differently once
// their never-taken memory-side branches are deleted; the change that settled the other switches shipped byte-identical kernels, so these
// two go with the next change to either kernel.
__device__ __forceinline__ bool hb_fresh_look(unsigned looks) { (void)looks; return false; }

// one lane waits until *word >= want; bounded; returns false when the run is being aborted
template <int SLEEP = 8>
__device__ __forceinline__ bool wait_ge(unsigned *flags, int word, unsigned want)
{
    const unsigned long long t0 = wall_clock64();
    for (;;) {
        if (ld_flag(flags + word) >= want) return true;
        if (ld_flag(flags + HB_FLAG_ABORT)) return false;
        if (wall_clock64() - t0 > HB_TIMEOUT_TICKS) {
            st_flag(flags + HB_FLAG_ABORT, 1u);
            st_flag(flags + 8, want); // (diagnostics: who gave up, hb_ctx.hip fetch_acc)
            hb_abort_log(flags, HB_LOG_WAIT_GE, true, (unsigned)word, want, ld_flag(flags + word));
            return false;
        }
        __builtin_amdgcn_s_sleep(SLEEP);
    }
}
