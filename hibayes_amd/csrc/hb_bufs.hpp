// hb_bufs.hpp — the one place device and pinned memory is allocated and freed. Needs nothing of HIP beyond
// <hip/hip_runtime.h>: tests/test_ownership_host.py compiles it against a stand-in for that header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../include/hibayes_gpu.h"

int hb_fail(int status, const std::string &msg); // sets the thread's last error (hb_ctx.hip)

#define HB_HIP(expr)                                                                         \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return hb_fail(HB_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)

// a call that has already reported its failure (hb_fail): pass its status on
#define HB_TRY(x)             \
    do {                      \
        const int _rc = (x);  \
        if (_rc) return _rc;  \
    } while (0)

// HB_HIP for an allocation into *p: refused, *p is null and the refusal does not show up again behind the next kernel launch (hipGetLastError)
#define HB_BUFS_ALLOC(expr)                                                                  \
    do {                                                                                     \
        *p = nullptr;                                                                        \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            *p = nullptr;                                                                    \
            (void)hipGetLastError();                                                         \
            return hb_fail(HB_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
        }                                                                                    \
    } while (0)

// what the process holds: live buffers and their bytes, device and pinned together (hb_debug_live_buffers). A buffer counts from its
// allocation to its free, whoever owns it in between.
inline std::atomic<int64_t> hb_live_count{0}, hb_live_bytes{0};
inline void hb_live_add(int64_t buffers, int64_t bytes)
{
    hb_live_count.fetch_add(buffers, std::memory_order_relaxed);
    hb_live_bytes.fetch_add(bytes, std::memory_order_relaxed);
}

// buffers that left their owner (hb_bufs::release) and are the caller's until hb_free_released: their sizes, for the count
inline std::mutex hb_released_mu;
inline std::unordered_map<void *, size_t> hb_released;

// The few MB of words that one workgroup publishes write-through while workgroups on OTHER XCDs poll them (dots, correction sums,
// changes of effect, move counts and lists, bounds, the flag block). HB_HANDOFF_ALLOC selects what kind of device memory they
// live in: 0 = plain hipMalloc (coarse-grained: cached in every XCD's L2 — the polls and stores carry sc1 to get past it),
// 1 = hipDeviceMallocUncached (MTYPE UC: no L2 copy anywhere, a store goes straight to the memory side), 2 = fine-grained
// (coherent across agents). Round 5's experiment on the lost store of DESIGN.md §9.0; the arrays are small, the genotypes, Gram
// blocks and everything streamed stay plain. Read once per process.
inline int hb_handoff_kind()
{
    static const int kind = [] {
        const char *e = getenv("HB_HANDOFF_ALLOC");
        return e ? std::max(0, std::min(2, atoi(e))) : 0;
    }();
    return kind;
}

inline std::string hb_dims(int64_t n) { return std::to_string(n) + " x " + std::to_string(n); } // "300 x 300", for hb_bufs::big's text

// the device and pinned allocations of one call, run or handle, freed on every way out. An owner that also holds a graph or a stream
// destroys the graph, calls clear() and destroys the stream, in that order. A refused allocation leaves the caller's pointer null.
struct hb_bufs {
    struct buf { void *p; size_t bytes; };
    std::vector<buf> dev, pinned;
    hb_bufs() = default;
    hb_bufs(const hb_bufs &) = delete;
    hb_bufs &operator=(const hb_bufs &) = delete;
    ~hb_bufs() { clear(); }
    void clear()
    {
        for (const buf &b : dev) { (void)hipFree(b.p); hb_live_add(-1, -(int64_t)b.bytes); }
        for (const buf &b : pinned) { (void)hipHostFree(b.p); hb_live_add(-1, -(int64_t)b.bytes); }
        dev.clear();
        pinned.clear();
    }
    template <typename T> int get(T **p, size_t count) // device memory, as hipMalloc leaves it
    {
        HB_BUFS_ALLOC(hipMalloc(reinterpret_cast<void **>(p), std::max<size_t>(count, 1) * sizeof(T)));
        keep(dev, *p, std::max<size_t>(count, 1) * sizeof(T));
        return HB_OK;
    }
    template <typename T> bool try_get(T **p, size_t count) // get() for a buffer the caller can do without: refused, *p is null and nothing is reported
    {
        *p = nullptr;
        if (hipMalloc(reinterpret_cast<void **>(p), std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) {
            *p = nullptr;
            (void)hipGetLastError();
            return false;
        }
        keep(dev, *p, std::max<size_t>(count, 1) * sizeof(T));
        return true;
    }
    template <typename T> int zeroed(T **p, size_t count, hipStream_t s) // device memory, zeroed on stream s
    {
        HB_TRY(get(p, count));
        HB_HIP(hipMemsetAsync(*p, 0, std::max<size_t>(count, 1) * sizeof(T), s));
        return HB_OK;
    }
    template <typename T> int pin(T **p, size_t count) // pinned host memory
    {
        HB_BUFS_ALLOC(hipHostMalloc(reinterpret_cast<void **>(p), std::max<size_t>(count, 1) * sizeof(T)));
        keep(pinned, *p, std::max<size_t>(count, 1) * sizeof(T));
        return HB_OK;
    }
    template <typename T> int handoff(T **p, size_t count, hipStream_t s) // hand-off memory (hb_handoff_kind), zeroed on stream s
    {
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        const int kind = hb_handoff_kind();
        if (kind == 0) HB_BUFS_ALLOC(hipMalloc(reinterpret_cast<void **>(p), bytes));
        else HB_BUFS_ALLOC(hipExtMallocWithFlags(reinterpret_cast<void **>(p), bytes, kind == 1 ? hipDeviceMallocUncached : hipDeviceMallocFinegrained));
        keep(dev, *p, bytes);
        HB_HIP(hipMemsetAsync(*p, 0, bytes, s));
        return HB_OK;
    }
    // a buffer whose size comes from the caller's n (what: "the " + hb_dims(n) + " matrix"): refused, the text tells who asked, for what
    // and how many GB
    template <typename T> int big(T **p, size_t count, const char *who, const std::string &what)
    {
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        *p = nullptr;
        if (hipMalloc(reinterpret_cast<void **>(p), bytes) != hipSuccess) {
            *p = nullptr;
            (void)hipGetLastError();
            char gb[48];
            snprintf(gb, sizeof gb, " needs %.1f GB on the device", 1e-9 * (double)bytes);
            return hb_fail(HB_ERR_HIP, std::string(who) + ": hipMalloc: out of memory — " + what + gb);
        }
        keep(dev, *p, bytes);
        return HB_OK;
    }
    template <typename T> void drop(T **p) // free *p now (device or pinned) and forget it; the caller's pointer is null afterwards
    {
        if (*p) {
            size_t bytes = 0;
            if (take(dev, *p, &bytes)) (void)hipFree(*p);
            else if (take(pinned, *p, &bytes)) (void)hipHostFree(*p);
            else return; // (not this owner's: left alone)
            hb_live_add(-1, -(int64_t)bytes);
        }
        *p = nullptr;
    }
    void give(hb_bufs &to, void *q) // q (device memory) is the other owner's from here
    {
        size_t bytes = 0;
        if (take(dev, q, &bytes)) to.dev.push_back({q, bytes});
    }
    void release(void *q) // the caller keeps q (device memory); hb_free_released frees it
    {
        size_t bytes = 0;
        if (!take(dev, q, &bytes)) return;
        std::lock_guard<std::mutex> lk(hb_released_mu);
        hb_released[q] = bytes;
    }

private:
    static void keep(std::vector<buf> &list, void *q, size_t bytes)
    {
        list.push_back({q, bytes});
        hb_live_add(1, (int64_t)bytes);
    }
    static bool take(std::vector<buf> &list, void *q, size_t *bytes)
    {
        for (size_t i = 0; i < list.size(); i++)
            if (list[i].p == q) {
                *bytes = list[i].bytes;
                list.erase(list.begin() + (std::ptrdiff_t)i);
                return true;
            }
        return false;
    }
};

// frees a device buffer that hb_bufs::release handed to the caller (hb_grm_free, hb_eig_release). ONLY those: nullptr and pointers it does not
// know are left alone, so a function that hands a buffer out must release() it, or the caller's free does nothing and the buffer leaks
inline void hb_free_released(void *q)
{
    size_t bytes = 0;
    {
        std::lock_guard<std::mutex> lk(hb_released_mu);
        const auto it = hb_released.find(q);
        if (it == hb_released.end()) return;
        bytes = it->second;
        hb_released.erase(it);
    }
    (void)hipFree(q);
    hb_live_add(-1, -(int64_t)bytes);
}

#undef HB_BUFS_ALLOC
