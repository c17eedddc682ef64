// hb_stedcplan.hpp — the merge tree of the device's tridiagonal divide and conquer (hb_stedc.hip): a pure function of n, the split
// points and STEDC_LEAF, so it compiles on the host and is tested there (hb_stedc_plan, tests/test_stedc_host.py; tests/stedc_restatement.py
// restates it).
//
// A split point i says that e_i is negligible: the rows up to i and from i + 1 on are independent parts. A part of at most STEDC_LEAF rows is a
// leaf; a longer one is halved, lo + (hi - lo) / 2 (the first half has the smaller share of an odd size), down to leaves. A merge's level is one
// more than the higher of its two children's, leaves being level 0: the merges of one level are disjoint, a merge's children are complete before
// its level starts, and all merges of a level can go in the same launches.
#pragma once
#include <stdint.h>
#include <vector>

#ifndef STEDC_LEAF
#define STEDC_LEAF 32 // rows of a leaf at most: the block one workgroup diagonalises in LDS (hb_stedc.hip's k_stedc_leaf is written for 32)
#endif

struct hb_stedc_merge {
    int32_t lo, mid, hi, level; // the children are [lo, mid) and [mid, hi); the tear is at e[mid - 1]
};

struct hb_stedc_tree {
    std::vector<int32_t> leaf_lo, leaf_hi;
    std::vector<hb_stedc_merge> merges; // children before parents
    int32_t levels = 0;                 // the highest level of a merge (0: leaves alone)
};

inline int hb_stedc_build(hb_stedc_tree &t, int32_t lo, int32_t hi, int32_t leaf)
{
    if (hi - lo <= leaf) {
        t.leaf_lo.push_back(lo);
        t.leaf_hi.push_back(hi);
        return 0;
    }
    const int32_t mid = lo + (hi - lo) / 2;
    const int a = hb_stedc_build(t, lo, mid, leaf), b = hb_stedc_build(t, mid, hi, leaf);
    const int level = 1 + (a > b ? a : b);
    t.merges.push_back({lo, mid, hi, level});
    return level;
}

// splits: ascending, each in [0, n - 1)
inline hb_stedc_tree hb_stedc_tree_of(int32_t n, const int32_t *splits, int32_t nsplit, int32_t leaf = STEDC_LEAF)
{
    hb_stedc_tree t;
    int32_t lo = 0;
    for (int32_t s = 0; s <= nsplit; s++) {
        const int32_t hi = s < nsplit ? splits[s] + 1 : n;
        const int level = hb_stedc_build(t, lo, hi, leaf);
        if (level > t.levels) t.levels = level;
        lo = hi;
    }
    return t;
}
