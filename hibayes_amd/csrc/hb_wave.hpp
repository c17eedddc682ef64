// hb_wave.hpp — what every unit with kernels uses of one 64-lane wave: the shuffle sum and the block sum built on it, a lane's double
// read as a scalar, the short vector types of the MFMA operands and 16-byte loads, HB_INF, and the four-genotype load of the int8 / 2-bit
// layouts. One text for the chain kernels' unit
// and the units beside it.
#pragma once
#include <hip/hip_runtime.h>

#define HB_INF __builtin_huge_val()

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef double d2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// block-wide sum, result valid in every thread; red must hold blockDim.x/64 entries. The wave sums are added in wave order: the
// order that the bit-for-bit tests of the sweeps and of both summary-level samplers rest on.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T *red)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    T s = 0;
    for (int i = 0; i < nw; i++) s += red[i];
    return s;
}

__device__ __forceinline__ double readlane_f64(double v, int k)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), k);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
    return __hiloint2double(hi, lo);
}

// four consecutive individuals (row0 a multiple of 4) of one column, one genotype per byte: from the int8 matrix, or expanded in
// registers from the 2-bit resident layout (individual 16 w + 4 k + b sits in bits [8 b + 2 k, 8 b + 2 k + 1] of word w)
__device__ __forceinline__ int hb_ld4(const int8_t *X, int64_t ld, const uint32_t *X2, int64_t ld2w, int64_t col, int64_t row0)
{
    if (X2) {
        const unsigned w = X2[col * ld2w + (row0 >> 4)];
        return (int)((w >> ((row0 & 12) >> 1)) & 0x03030303u);
    }
    return *reinterpret_cast<const int *>(X + col * ld + row0);
}
