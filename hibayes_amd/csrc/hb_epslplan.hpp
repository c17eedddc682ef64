// hb_epslplan.hpp — the schedule of the single-step model's Gibbs pass (hb_epsl.hip) and the validation of its arguments: pure
// functions of the sparsity pattern, so they compile on the host and are tested there (hb_epsl_plan / hb_epsl_check, tests/test_epsl_host.py;
// tests/epsl_restatement.py restates the levels).
//
// The pass of src/solver.cpp:131-140 visits the rows i = 0 .. q - 1 in order; row i reads x_j for the stored entries j of column i of the
// symmetric matrix — new values for j < i, old ones for j > i. With
//     level(i) = 1 + max level(j) over the stored j < i        (0 where there is none)
// every stored pair (i, j), j < i, has level(j) < level(i): evaluating the levels in ascending order, the rows of one level in any order or at
// once, gives every row the values the sequential pass gives it — the new ones of its lower neighbours (all in earlier levels), the old ones of
// its higher neighbours (all in later levels). Two rows of one level share no stored entry.
//
// A step is one level: its rows with a short column first (a lane each), then those with a long one (a wave each), both in ascending row order.
// A launch is either one wide step over the chip, or a run of consecutive narrow steps that ONE workgroup walks with a barrier between them.
// Ordering between launches comes from the stream alone; nothing in the pass waits for another workgroup.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#define EPSL_WAVE_MIN 33     // stored entries of a column from which the row takes a wave (row_mode 0)
// lanes of work (lane rows + 64 * wave rows) up to which a step stays in a single-workgroup launch (sched_mode 0): one workgroup of 256 lanes, so
// every row of a narrow step has a lane or a wave of its own at once. Measured (profiles/epsl_timing.txt): a step costs that workgroup a few
// dependent memory round trips and a barrier, a wide launch about 12 us; at 2048 a workgroup walking 1 800-row levels lost to a host thread.
#define EPSL_NARROW_WORK 256

struct hb_epsl_step {
    int32_t level, lane0, nlane, wave0, nwave; // rows[lane0 .. lane0 + nlane) take a lane each, rows[wave0 .. wave0 + nwave) a wave each
};
struct hb_epsl_launch {
    int32_t kind, s0, s1; // kind 0: one workgroup walks steps [s0, s1) with a barrier after each; kind 1: step s0 over the chip (s1 = s0 + 1)
};
struct hb_epsl_sched {
    int32_t q = 0, levels = 0, max_col = 0;
    std::vector<int32_t> level, rows;
    std::vector<hb_epsl_step> steps;
    std::vector<hb_epsl_launch> launches;
};

// sched_mode 0: by EPSL_NARROW_WORK; 1: every step in single-workgroup launches (one launch); 2: every step wide.
// row_mode 0: by EPSL_WAVE_MIN; 1: a lane for every row; 2: a wave for every row.   (1 and 2 are the tests' debug settings: same result)
inline hb_epsl_sched hb_epsl_plan_of(int32_t q, const int64_t *indptr, const int32_t *indices, int sched_mode = 0, int row_mode = 0)
{
    hb_epsl_sched p;
    p.q = q;
    p.level.assign(q, 0);
    for (int32_t i = 0; i < q; i++) {
        int32_t lv = 0;
        for (int64_t k = indptr[i]; k < indptr[i + 1]; k++) {
            const int32_t j = indices[k];
            if (j < i) lv = std::max(lv, p.level[j] + 1);
        }
        p.level[i] = lv;
        p.levels = std::max(p.levels, lv + 1);
        p.max_col = std::max<int32_t>(p.max_col, (int32_t)(indptr[i + 1] - indptr[i]));
    }
    auto is_wave = [&](int32_t i) { return row_mode == 2 || (row_mode == 0 && indptr[i + 1] - indptr[i] >= EPSL_WAVE_MIN); };
    // counting sort by (level, wave?) keeps the rows of a group in ascending order
    std::vector<int32_t> cnt(2 * (size_t)p.levels + 1, 0);
    for (int32_t i = 0; i < q; i++) cnt[2 * (size_t)p.level[i] + (is_wave(i) ? 1 : 0) + 1]++;
    for (size_t g = 0; g < 2 * (size_t)p.levels; g++) cnt[g + 1] += cnt[g];
    p.rows.assign(q, 0);
    {
        std::vector<int32_t> at(cnt.begin(), cnt.end() - 1);
        for (int32_t i = 0; i < q; i++) p.rows[at[2 * (size_t)p.level[i] + (is_wave(i) ? 1 : 0)]++] = i;
    }
    for (int32_t l = 0; l < p.levels; l++) {
        const int32_t a = cnt[2 * (size_t)l], b = cnt[2 * (size_t)l + 1], c = cnt[2 * (size_t)l + 2];
        p.steps.push_back({l, a, b - a, b, c - b});
    }
    for (int32_t s = 0; s < (int32_t)p.steps.size(); s++) {
        const int64_t work = (int64_t)p.steps[s].nlane + 64 * (int64_t)p.steps[s].nwave;
        const bool narrow = sched_mode == 1 || (sched_mode == 0 && work <= EPSL_NARROW_WORK);
        if (!narrow) p.launches.push_back({1, s, s + 1});
        else if (!p.launches.empty() && p.launches.back().kind == 0 && p.launches.back().s1 == s) p.launches.back().s1 = s + 1;
        else p.launches.push_back({0, s, s + 1});
    }
    return p;
}

// The arguments of the block: G (q x q, the full symmetric matrix in canonical CSC, 0-based) and index (ne entries, 1-based as the
// reference's epsl_index, the individual of each of the LAST ne records). Returns an empty string, or what is wrong.
inline std::string hb_epsl_check_args(int32_t q, int32_t ne, const int64_t *indptr, const int32_t *indices, const double *data, const uint32_t *index,
                                      int32_t n)
{
    if (q < 1 || !indptr || !indices || !data) return "epsl_Gi: an empty descriptor (q, indptr, indices, data)";
    if (ne < 1 || ne > n || !index) return "epsl_index: between 1 and n records belong to the epsilon term";
    for (int32_t r = 0; r < ne; r++)
        if (index[r] < 1 || index[r] > (uint32_t)q) return "epsl_index: an index is outside 1 .. q (the columns of epsl_Gi)";
    if (indptr[0] != 0) return "epsl_Gi: indptr must start at 0";
    for (int32_t i = 0; i < q; i++)
        if (indptr[i + 1] < indptr[i]) return "epsl_Gi: indptr must not decrease";
    for (int32_t i = 0; i < q; i++) {
        bool diag = false;
        for (int64_t k = indptr[i]; k < indptr[i + 1]; k++) {
            const int32_t j = indices[k];
            if (j < 0 || j >= q) return "epsl_Gi: a row index is outside 0 .. q - 1";
            if (k > indptr[i] && indices[k - 1] >= j) return "epsl_Gi: the row indices of a column must be sorted and unique (canonical CSC)";
            if (!std::isfinite(data[k])) return "epsl_Gi: a stored value is not finite";
            if (j == i) {
                diag = true;
                if (!(data[k] > 0.0)) return "epsl_Gi: the diagonal must be positive";
            }
        }
        if (!diag) return "epsl_Gi: the diagonal must be positive";
    }
    // symmetric: entry (j, i) of column i has its mirror (i, j) in column j, with the same value
    for (int32_t i = 0; i < q; i++)
        for (int64_t k = indptr[i]; k < indptr[i + 1]; k++) {
            const int32_t j = indices[k];
            if (j == i) continue;
            const int32_t *b = indices + indptr[j], *e = indices + indptr[j + 1];
            const int32_t *f = std::lower_bound(b, e, i);
            if (f == e || *f != i || data[f - indices] != data[k]) return "epsl_Gi: the matrix must be symmetric, pattern and values (both triangles stored)";
        }
    return std::string();
}
