// hb_mma.hpp — the matrix-core tile loops the dense units share (hb_gram.hip, hb_ldmat.hip, hb_grm.hip, hb_eig.hip, hb_stedc.hip): the int8
// 32x32x32 wave step with its accumulator layout, the LDS-staged 256 x 256 workgroup loop built on it, the fp64 16x16x4 wrapper with its
// layout, and the decode of a block index into a tile of a lower triangle. One text each, so that the bank-conflict stride, the C/D mappings
// and the triangle decode are fixed in one place.
// Some of the units above are compiled with floating-point contraction off and some with it on. Nothing here can tell the difference: the
// header holds MFMA builtins, integer arithmetic and loads only (tri_tile's square root seeds a search that integers then settle).
#pragma once
#include "hb_wave.hpp"

// ---------------------------------------------------------------------------------------------------------------------------------
// int8: v_mfma_i32_32x32x32_i8, a wave's 64 x 64 tile as 2 x 2 MFMA tiles of 32 x 32
// ---------------------------------------------------------------------------------------------------------------------------------
// Operands: both are K-contiguous columns of int8, cs bytes apart. Lane l reads 16 bytes of column l & 31 of a 32-wide sub-tile, the k values
// 16 (l >> 5) .. + 15 of the step's 32; the second sub-tile sits 32 columns on.
// C/D layout: lane l holds, in register r of acc[a][b], the entry whose A-operand column (the row) is 32 a + (r & 3) + 8 (r >> 2) + 4 (l >> 5)
// and whose B-operand column (the column) is 32 b + (l & 31).
__device__ __forceinline__ int64_t mma_i8_operand(int lane, int64_t cs) { return (int64_t)(lane & 31) * cs + 16 * (lane >> 5); }
__device__ __forceinline__ int mma_i8_row(int a, int r, int lane) { return 32 * a + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }
__device__ __forceinline__ int mma_i8_col(int b, int lane) { return 32 * b + (lane & 31); }

__device__ __forceinline__ void mma_i8_zero(v16i (&acc)[2][2])
{
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0;
}

// acc += A' B over 32 k values; pa / pb: this lane's 16 bytes of the first sub-tile of either operand (global memory or LDS)
__device__ __forceinline__ void mma_i8_step(v16i (&acc)[2][2], const void *pa, const void *pb, int64_t cs)
{
    const char *xa = static_cast<const char *>(pa), *xb = static_cast<const char *>(pb);
    const v4i a0 = *reinterpret_cast<const v4i *>(xa);
    const v4i a1 = *reinterpret_cast<const v4i *>(xa + 32 * cs);
    const v4i b0 = *reinterpret_cast<const v4i *>(xb);
    const v4i b1 = *reinterpret_cast<const v4i *>(xb + 32 * cs);
    acc[0][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, acc[1][1], 0, 0, 0);
}

// ---- the staged loop: a 256 x 256 tile per workgroup of 16 waves (4 x 4 wave tiles of 64 x 64: wave >> 2 down the A operand, wave & 3 along
// the B operand). Per 64-row step the 256 + 256 operand columns are staged through LDS once — 16-byte global loads into registers one step
// ahead, ds_write_b128 with an 80-byte column stride so that the MFMA operand reads are bank-conflict free — instead of being re-read from
// global memory by every wave tile.
constexpr int MMA_T = 256; // columns of either operand per workgroup
constexpr int MMA_KS = 64; // rows per step
constexpr int MMA_CS = 80; // bytes per staged column: 64 + 16
// staging: thread -> (column tid / 4, 16-byte part tid % 4) of both operand tiles
__device__ __forceinline__ int mma_stage_col(int tid) { return tid >> 2; }
__device__ __forceinline__ int mma_stage_part(int tid) { return tid & 3; }

// acc += A' B over ld rows (a multiple of 64). ga / gb: row 16 * mma_stage_part(tid) of the thread's column mma_stage_col(tid) of either
// operand tile; sa / sb: MMA_T * MMA_CS bytes of LDS each, 16-byte aligned. All 1024 threads of the workgroup call it together.
__device__ __forceinline__ void mma_i8_staged(v16i (&acc)[2][2], const int8_t *__restrict__ ga, const int8_t *__restrict__ gb, int64_t ld, char *sa, char *sb,
                                              int tid)
{
    const int wave = tid >> 6, lane = tid & 63;
    const int slot = mma_stage_col(tid) * MMA_CS + mma_stage_part(tid) * 16;
    const char *ra = sa + (wave >> 2) * 64 * MMA_CS + mma_i8_operand(lane, MMA_CS);
    const char *rb = sb + (wave & 3) * 64 * MMA_CS + mma_i8_operand(lane, MMA_CS);
    v4i na = *reinterpret_cast<const v4i *>(ga), nb = *reinterpret_cast<const v4i *>(gb);
    for (int64_t kk = 0; kk < ld; kk += MMA_KS) {
        __syncthreads(); // everybody is done reading the previous step
        *reinterpret_cast<v4i *>(sa + slot) = na;
        *reinterpret_cast<v4i *>(sb + slot) = nb;
        __syncthreads();
        if (kk + MMA_KS < ld) { // next step's operands travel while this one is multiplied
            na = *reinterpret_cast<const v4i *>(ga + kk + MMA_KS);
            nb = *reinterpret_cast<const v4i *>(gb + kk + MMA_KS);
        }
#pragma unroll
        for (int ks = 0; ks < MMA_KS; ks += 32) mma_i8_step(acc, ra + ks, rb + ks, MMA_CS);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// fp64: v_mfma_f64_16x16x4_f64, a wave's 32 x 32 tile as 2 x 2 MFMA tiles of 16 x 16
// ---------------------------------------------------------------------------------------------------------------------------------
// Lane l gives A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; it receives, in register r, D[row (l >> 4) + 4 r][col l & 15].
// With acc[a][b] = mfma_f64(x[b], y[a], acc[a][b]) the entry in register r of acc[a][b] has row 16 b + (l >> 4) + 4 r (x's index) and column
// 16 a + (l & 15) (y's index): the kernels let the columns of D run along the index that is contiguous in memory.
typedef double v4d __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4d mfma_f64(double a, double b, v4d acc) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0); }
__device__ __forceinline__ int mma_f64_row(int b, int r, int lane) { return 16 * b + (lane >> 4) + 4 * r; }
__device__ __forceinline__ int mma_f64_col(int a, int lane) { return 16 * a + (lane & 15); }

__device__ __forceinline__ void mma_f64_zero(v4d (&acc)[2][2])
{
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) acc[a][b] = (v4d){0.0, 0.0, 0.0, 0.0};
}

// ---------------------------------------------------------------------------------------------------------------------------------
// x = bi (bi + 1) / 2 + bj with 0 <= bj <= bi: the tile (bi, bj) of a lower triangle from a linear block index
// ---------------------------------------------------------------------------------------------------------------------------------
// 8 x + 1 is formed in integers and is exact as a double (x < 2^49); the root may still be one off either way, which the two loops correct.
__host__ __device__ inline void tri_tile(long long x, int *bi, int *bj)
{
    long long i = (long long)((sqrt((double)(8 * x + 1)) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= x) i++;
    while (i * (i + 1) / 2 > x) i--;
    *bi = (int)i;
    *bj = (int)(x - i * (i + 1) / 2);
}
