// kernels_linear.hip.h -- linear layers: a dense integer matrix applied to vectors of ciphertexts.
//   y[set][j][i] = sum_k (uint32)W[j][k] x[set][k][i] + (i == words - 1 ? bias[j] : 0)   mod 2^32,   0 <= j < rows, 0 <= i < words
// Word arithmetic only, no key: every word is exact and the same for every launch shape.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "launch_plan.h"

namespace cufhe_amd {

constexpr int kLinearTJ = plan::kLinearRowTile;
constexpr int kLinearU = plan::kLinearUnroll;

// The device copy of a layer: the weights by row tile, [row_tiles][cols][kLinearTJ] with zero rows behind `rows`, so that the TJ weights a
// wave needs for one k are 64 contiguous bytes; the bias padded to the same rows.
inline size_t linear_weight_words(size_t rows, size_t cols) { return (rows + kLinearTJ - 1) / kLinearTJ * kLinearTJ * cols; }
inline size_t linear_weight_index(size_t row, size_t k, size_t cols) { return (row / kLinearTJ * cols + k) * kLinearTJ + row % kLinearTJ; }

// Ciphertext pointers come out of the pointer tables: the compiler cannot know their address space and would use flat loads and stores,
// which also wait on the LDS counter.  They are device (global) memory by the entry points' contract.
using LinearInPtr = const __attribute__((address_space(1))) uint32_t*;
using LinearOutPtr = __attribute__((address_space(1))) uint32_t*;

// Wave = (row tile, chunk of 64 word indices, set) in the numbering of plan::plan_linear; lane = one word index i; acc[j] = output row
// tile * TJ + j at i.  Per k: one coalesced dword load of x_k[i] (the pointer through a scalar load: ins is indexed by wave-uniform
// values only) and TJ multiply-adds whose weights are wave-uniform -- the wave's number is made provably so by readfirstlane, and the
// compiler then fetches them with scalar loads into SGPRs.  k is walked U at a time so that U loads are in flight before the first
// product.  A lane behind the last word of the ciphertext (the partial last chunk) reads word words - 1 instead and stores nothing.
// ins: [sets][cols] pointers, outs: [sets][rows]; no output may alias an input (the host refuses it): other waves still read them.
__global__ __launch_bounds__(plan::kLinearWaveWords * plan::kLinearMaxWaves) void linear_kernel(
    const uint32_t* const* __restrict__ ins, uint32_t* const* __restrict__ outs, const int32_t* __restrict__ weights,
    const uint32_t* __restrict__ bias, int rows, int cols, int words, int row_tiles, int chunks, long waves)
{
    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / plan::kLinearWaveWords));
    const long wave = plan::linear_wave_of((long)blockIdx.x, wave_in_block, (int)(blockDim.x / plan::kLinearWaveWords));
    if (wave >= waves) return;
    const int tile = plan::linear_wave_tile(wave, row_tiles);
    const int chunk = plan::linear_wave_chunk(wave, row_tiles, chunks);
    const long set = plan::linear_wave_set(wave, row_tiles, chunks);
    const int i = plan::linear_word(chunk, (int)(threadIdx.x % plan::kLinearWaveWords));
    const bool live = i < words;
    const int ir = live ? i : words - 1;

    const uint32_t* const* __restrict__ x = ins + set * cols;
    const uint32_t* __restrict__ w = (const uint32_t*)weights + (size_t)tile * cols * kLinearTJ;
    uint32_t acc[kLinearTJ];
#pragma unroll
    for (int j = 0; j < kLinearTJ; j++) acc[j] = 0u;

    int k = 0;
    for (; k + kLinearU <= cols; k += kLinearU) {
        uint32_t xv[kLinearU];
#pragma unroll
        for (int u = 0; u < kLinearU; u++) xv[u] = ((LinearInPtr)x[k + u])[ir];
#pragma unroll
        for (int u = 0; u < kLinearU; u++)
#pragma unroll
            for (int j = 0; j < kLinearTJ; j++) acc[j] += w[(size_t)(k + u) * kLinearTJ + j] * xv[u];
    }
    for (; k < cols; k++) {
        const uint32_t xv = ((LinearInPtr)x[k])[ir];
#pragma unroll
        for (int j = 0; j < kLinearTJ; j++) acc[j] += w[(size_t)k * kLinearTJ + j] * xv;
    }

    if (!live) return;
    uint32_t* const* __restrict__ y = outs + set * rows;
#pragma unroll
    for (int j = 0; j < kLinearTJ; j++) {
        const int row = plan::linear_row(tile, j);
        if (row < rows) ((LinearOutPtr)y[row])[i] = acc[j] + (i == words - 1 ? bias[row] : 0u);
    }
}

}  // namespace cufhe_amd
