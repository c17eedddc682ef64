// hb_imputeplan.hpp — the geometry of ssbrm()'s device imputation (hb_impute.hip) and the validation of its matrices: pure
// functions of sizes and sparsity patterns, so they compile on the host and are tested there (tests/test_impute_host.py compiles this header
// with g++).
//
// The solve is a batched Jacobi-preconditioned conjugate gradient on A^-1_nn X = -A^-1_ng M. A block vector is q rows of W doubles, W a
// multiple of 64: a wave owns a row, a lane one right-hand side of it. Every per-column sum over the q rows is formed as `parts` partial sums
// over runs of `rows_per_part` consecutive rows — one workgroup of IMP_WAVES waves per run, wave w adding the rows w, w + IMP_WAVES, ... of
// its run in ascending order, the waves' sums then added in wave order, the parts in the order of imp_colsums (hb_impute.hip). That
// partition is a function of q ALONE: a column's sums do not depend on the block width, on the column's lane or on what else is in the block.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#define IMP_WAVES 16                        // waves per workgroup, every kernel of the unit (1024 threads)
#define IMP_MAX_PARTS 512                   // partial sums per column at most: every workgroup of an update kernel re-adds them all
#define IMP_MAX_WIDTH 512                   // the widest block
#define IMP_CACHE_BYTES (256ll << 20)       // the Infinity Cache
// blocks of q x W doubles that one iteration streams between two gathers of the same row of p: the product writes Ap (1); the first update
// reads p and Ap and reads and writes x and r (6); the second reads r and reads and writes p (3)
#define IMP_STREAMED_BLOCKS 10
#define IMP_DEVICE_BLOCKS 5                 // x, r, p, Ap, b resident for a solve (Ap doubles as the staging of the result)

struct hb_impute_plan {
    int32_t ok = 0;
    int32_t width = 0;                      // W
    int32_t groups = 0;                     // W / 64: the y dimension of every grid
    int32_t parts = 0, rows_per_part = 0;   // the x dimension of every grid, and the rows of one workgroup
    int32_t cached = 0;                     // the p block fits the Infinity Cache beside one iteration's streamed traffic
    int64_t device_bytes = 0;               // what a solve at this width allocates
    std::string why;                        // !ok: what does not fit
};

// the partition of the q rows into partial sums: a function of q alone
inline void hb_impute_partition(int32_t q, int32_t *parts, int32_t *rows_per_part)
{
    const int64_t want = std::min<int64_t>(IMP_MAX_PARTS, ((int64_t)q + IMP_WAVES - 1) / IMP_WAVES);
    int64_t rows = ((int64_t)q + want - 1) / std::max<int64_t>(want, 1);
    rows = (rows + IMP_WAVES - 1) / IMP_WAVES * IMP_WAVES; // every wave of a run has the same number of turns (but the last run's)
    *rows_per_part = (int32_t)rows;
    *parts = (int32_t)(((int64_t)q + rows - 1) / rows);
}

// device bytes of a solve at width W: the blocks, the chunk of M in both layouts, the partial sums, the matrices
inline int64_t hb_impute_bytes(int32_t q, int64_t nnz_nn, int32_t n_g, int64_t nnz_ng, int32_t W)
{
    int32_t parts, rows;
    hb_impute_partition(q, &parts, &rows);
    const int64_t block = (int64_t)q * W * 8;
    const int64_t m = 2 * (int64_t)n_g * W * 8;
    const int64_t sums = 5 * (int64_t)parts * W * 8 + 16 * (int64_t)W * 8;
    const int64_t mats = (nnz_nn + nnz_ng) * 12 + 2 * ((int64_t)q + 1) * 8 + (int64_t)q * 8;
    return IMP_DEVICE_BLOCKS * block + m + sums + mats;
}

// W for a solve of `cols` right-hand sides: the widest block, no wider than the columns need, whose p stays within the Infinity Cache beside
// one iteration's streamed traffic; 64 where none does (the gathers then come from HBM, a row at a time); narrower again until the solve fits
// free_bytes of device memory; refused where the narrowest does not.
inline hb_impute_plan hb_impute_plan_of(int32_t q, int64_t nnz_nn, int32_t n_g, int64_t nnz_ng, int32_t cols, int64_t free_bytes)
{
    hb_impute_plan p;
    if (q < 1 || n_g < 1 || cols < 1 || nnz_nn < q || nnz_ng < 0) {
        p.why = "hb_impute: empty system (q, n_g, columns)";
        return p;
    }
    const int32_t need = (int32_t)std::min<int64_t>(IMP_MAX_WIDTH, ((int64_t)cols + 63) / 64 * 64);
    int32_t W = 64;
    for (int32_t w = need; w >= 64; w -= 64)
        if ((int64_t)q * w * 8 * (1 + IMP_STREAMED_BLOCKS) <= IMP_CACHE_BYTES) {
            W = w;
            p.cached = 1;
            break;
        }
    while (W > 64 && hb_impute_bytes(q, nnz_nn, n_g, nnz_ng, W) > free_bytes) W -= 64;
    p.device_bytes = hb_impute_bytes(q, nnz_nn, n_g, nnz_ng, W);
    if (p.device_bytes > free_bytes) {
        p.why = "hb_impute: the narrowest block (64 columns) needs " + std::to_string(p.device_bytes >> 20) + " MiB of device memory, " +
                std::to_string(free_bytes >> 20) + " MiB are free";
        return p;
    }
    if ((int64_t)q * W * 8 * (1 + IMP_STREAMED_BLOCKS) > IMP_CACHE_BYTES) p.cached = 0;
    p.width = W;
    p.groups = W / 64;
    hb_impute_partition(q, &p.parts, &p.rows_per_part);
    p.ok = 1;
    return p;
}

// canonical compressed storage: indptr from 0, not decreasing; indices of a run sorted, unique, inside 0 .. minor - 1; finite values
inline std::string hb_impute_check_storage(const char *name, int32_t major, int32_t minor, const int64_t *indptr, const int32_t *indices,
                                           const double *data)
{
    const std::string n(name);
    if (indptr[0] != 0) return n + ": indptr must start at 0";
    for (int32_t i = 0; i < major; i++)
        if (indptr[i + 1] < indptr[i]) return n + ": indptr must not decrease";
    for (int32_t i = 0; i < major; i++)
        for (int64_t k = indptr[i]; k < indptr[i + 1]; k++) {
            const int32_t j = indices[k];
            if (j < 0 || j >= minor) return n + ": an index is outside its range";
            if (k > indptr[i] && indices[k - 1] >= j) return n + ": the indices of a row or column must be sorted and unique";
            if (!std::isfinite(data[k])) return n + ": a stored value is not finite";
        }
    return std::string();
}

// A_nn (q x q, CSC, both triangles) and A_ng (ng_rows x n_g, CSR). Returns an empty string, or what is wrong.
inline std::string hb_impute_check_args(int32_t q, const int64_t *nn_indptr, const int32_t *nn_indices, const double *nn_data, int32_t ng_rows,
                                        int32_t n_g, const int64_t *ng_indptr, const int32_t *ng_indices, const double *ng_data)
{
    if (q < 1 || !nn_indptr || !nn_indices || !nn_data) return "A_nn: an empty matrix (q, indptr, indices, data)";
    if (n_g < 1 || ng_rows < 1 || !ng_indptr || !ng_indices || !ng_data) return "A_ng: an empty matrix (rows, n_g, indptr, indices, data)";
    if (ng_rows != q) return "A_ng must have as many rows as A_nn (" + std::to_string(ng_rows) + " against " + std::to_string(q) + ")";
    std::string e = hb_impute_check_storage("A_nn", q, q, nn_indptr, nn_indices, nn_data);
    if (!e.empty()) return e;
    e = hb_impute_check_storage("A_ng", q, n_g, ng_indptr, ng_indices, ng_data);
    if (!e.empty()) return e;
    for (int32_t i = 0; i < q; i++) {
        const int32_t *b = nn_indices + nn_indptr[i], *en = nn_indices + nn_indptr[i + 1];
        const int32_t *f = std::lower_bound(b, en, i);
        if (f == en || *f != i || !(nn_data[f - nn_indices] > 0.0)) return "A_nn: the diagonal must be positive (row " + std::to_string(i) + ")";
    }
    // symmetric: entry (j, i) of column i has its mirror (i, j) in column j, with the same value bits
    for (int32_t i = 0; i < q; i++)
        for (int64_t k = nn_indptr[i]; k < nn_indptr[i + 1]; k++) {
            const int32_t j = nn_indices[k];
            if (j == i) continue;
            const int32_t *b = nn_indices + nn_indptr[j], *en = nn_indices + nn_indptr[j + 1];
            const int32_t *f = std::lower_bound(b, en, i);
            if (f == en || *f != i)
                return "A_nn must equal its transpose in pattern: (" + std::to_string(j) + ", " + std::to_string(i) + ") is stored, its mirror is not";
            uint64_t u, v;
            std::memcpy(&u, &nn_data[f - nn_indices], 8);
            std::memcpy(&v, &nn_data[k], 8);
            if (u != v)
                return "A_nn must equal its transpose in value bits: (" + std::to_string(j) + ", " + std::to_string(i) + ") differs from its mirror";
        }
    return std::string();
}
