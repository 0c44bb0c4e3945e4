// kernels_pack.hip.h -- TLWE packing: lvl0 TLWEs into chosen coefficients of a lvl1 TRLWE.  One exact
// table-sum key switch lvl0 -> TRLWE in the structure of private_keyswitch_kernel (kernels_pks.hip.h), with the rotation X^pos done
// at write-out.  Integer arithmetic mod 2^32 only: every word is deterministic and the same for every launch shape.
//   PackKS(x) = (0, b X^0) - sum_i sum_j [a_ij != 0] K[i][j][a_ij - 1],   a_ij = ((x[i] + 2^15) >> (32 - 2 (j + 1))) & 3
//   out[o]    = sum over the inputs m with dst[m] = o of X^pos[m] PackKS(in[m])
#pragma once
#include "kernels_common.hip.h"
#include "launch_plan.h"

namespace cufhe_amd {

// the library's own choice (TFHEpp's numbers for this key switch are not known here): t = 8 unsigned digits of basebit = 2
constexpr int kPackT = 8;
constexpr int kPackBasebit = 2;
constexpr int kPackNumBase = (1 << kPackBasebit) - 1;      // 3 rows per (i, j): digit v = 1 .. 3
constexpr int kPackRowWords = 2 * kN;                      // one TRLWE row: k + 1 = 2 polynomials of N = 1024
constexpr size_t kPackKeyWords = (size_t)kLvl0N * kPackT * kPackNumBase * kPackRowWords;      // K[i][j][v - 1][k + 1][N]
static_assert(kPackKeyWords == 30965760, "123.9 MB of uint32");
constexpr uint32_t kPackRound = 1u << (32 - kPackT * kPackBasebit - 1);
static_assert(kPackT * kPackBasebit < 32, "the rounding bit lies below the digits");

constexpr int kPackThreads = 256;
constexpr int kPackTile = 64;
constexpr int kPackIBlock = 16;            // input words whose digits are staged per pass
constexpr int kPackChunks = kPackRowWords / kPackThreads;  // 8
constexpr plan::PackGeometry kPackGeometry{kPackTile, kPackChunks, kLvl0N, kPackIBlock};
static_assert(kN % kPackThreads == 0, "a chunk lies inside one polynomial");

// Workgroup = (chunk c of 256 of the 2N row words, tile of up to kPackTile inputs, slice of i); thread = one row word of every input
// of the tile, kept in registers.  For each (i, j) the thread loads its word of the 3 candidate rows once into its own column of LDS,
// row 0 = 0, and every input of the tile adds the row its digit picks: the digit is the same for all lanes (an LDS broadcast), so the
// reads are conflict-free and nothing branches.  Write-out: row word e = p N + k of input m goes to coefficient (k + pos[m]) mod N of
// polynomial p of out[dst[m]], negated on wrap, by vector atomicAdd into the zeroed outputs (the host zeroes all of them first):
// uint32 wrap-around addition is order-free, so slices, tiles and inputs that share an output may arrive in any order.  The thread
// that holds row word N (coefficient 0 of the b polynomial) in slice 0 also adds the input's b word, which lands at coefficient pos.
// dst_pos: [2][count] -- dst then pos, checked by the host: 0 <= dst < count_out, 0 <= pos < N.
__global__ __launch_bounds__(kPackThreads) void pack_keyswitch_kernel(
    const uint32_t* __restrict__ in, int count, const int32_t* __restrict__ dst_pos, const uint32_t* __restrict__ key,
    uint32_t* __restrict__ out, int tiles, int slices)
{
    __shared__ uint32_t rows[(kPackNumBase + 1) * kPackThreads];
    __shared__ __attribute__((aligned(16))) uint8_t dig[kPackIBlock * kPackT * kPackTile];
    const int tid = threadIdx.x;
    const int c = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int slice = blockIdx.y;
    const int t0 = (int)plan::pack_tile_first(tile, kPackTile);
    const int nt = plan::pack_tile_inputs(tile, kPackTile, count);
    const int i_begin = plan::pack_slice_begin(slice, slices, kLvl0N), i_end = plan::pack_slice_begin(slice + 1, slices, kLvl0N);

    uint32_t acc[kPackTile];
#pragma unroll
    for (int t = 0; t < kPackTile; t++) acc[t] = 0u;
    rows[tid] = 0u;
    uint32_t* const col = rows + tid;
    const uint32_t* kbase = key + c * kPackThreads + tid;

    for (int ib = i_begin; ib < i_end; ib += kPackIBlock) {
        const int ni = min(kPackIBlock, i_end - ib);
        __syncthreads();                   // the digits of the previous block have been read
        for (int e = tid; e < ni * kPackTile; e += kPackThreads) {
            const int ii = e / kPackTile, t = e % kPackTile;
            const uint32_t a = t < nt ? in[(size_t)(t0 + t) * kLvl0Words + ib + ii] + kPackRound : 0u;
#pragma unroll
            for (int j = 0; j < kPackT; j++) dig[(ii * kPackT + j) * kPackTile + t] = (uint8_t)((a >> (32 - kPackBasebit * (j + 1))) & kPackNumBase);
        }
        __syncthreads();
        for (int ii = 0; ii < ni; ii++) {
            const uint32_t* krow_i = kbase + (size_t)(ib + ii) * kPackT * kPackNumBase * kPackRowWords;
            for (int j = 0; j < kPackT; j++) {
                const uint32_t* krow = krow_i + (size_t)j * kPackNumBase * kPackRowWords;
                uint32_t v[kPackNumBase];
#pragma unroll
                for (int k = 0; k < kPackNumBase; k++) v[k] = krow[k * kPackRowWords];
#pragma unroll
                for (int k = 0; k < kPackNumBase; k++) col[(k + 1) * kPackThreads] = v[k];     // this thread's column only: no barrier
                const uint32_t* dg = (const uint32_t*)(dig + (ii * kPackT + j) * kPackTile);
#pragma unroll
                for (int q = 0; q < kPackTile / 4; q++) {
                    if (4 * q < nt) {              // uniform
                        const uint32_t w = dg[q];  // the same address in every lane: a broadcast
#pragma unroll
                        for (int b = 0; b < 4; b++) acc[4 * q + b] += col[((w >> (8 * b)) & 0xffu) * kPackThreads];
                    }
                }
            }
        }
    }
    const int e = c * kPackThreads + tid;          // row word: polynomial e / N, coefficient e % N
    const int poly = e / kN, k = e % kN;
    const bool holds_b = slice == 0 && e == kN;
#pragma unroll
    for (int t = 0; t < kPackTile; t++) {
        if (t >= nt) continue;
        const int m = t0 + t;
        const int d = dst_pos[m], pos = dst_pos[count + m];
        uint32_t val = 0u - acc[t];
        if (holds_b) val += in[(size_t)m * kLvl0Words + kLvl0N];
        const int kk = k + pos;
        if (kk >= kN) val = 0u - val;
        atomicAdd(out + (size_t)d * kPackRowWords + poly * kN + (kk & (kN - 1)), val);
    }
}

// The recorded packs of one dependence level (pack.inc.h: lower_pack_ops) in one launch: the same workgroup over the CONCATENATION of
// their terms, each term's operands named by a descriptor instead of in + m stride / out + dst 2N, so that inputs are read where the
// gates left them and a tile may hold terms of several outputs.  Everything else is pack_keyswitch_kernel, which stays as it is (a
// sibling, not a shared body: the batch kernel's code does not move).  A thread stages digits of ONE tile slot only (e % kPackTile is
// tid % kPackTile for every e it visits), so it keeps that term's input pointer in a register: the gather has the batch kernel's lane
// pattern, tile index fastest, one row per lane.
struct PackDesc { const uint32_t* in; uint32_t* out; int32_t pos; };      // pos checked by the host: 0 <= pos < N

// outs[count]: the level's distinct output TRLWEs, scattered; one workgroup zeroes one of them (rows are 16-byte aligned device slots)
__global__ __launch_bounds__(kPackThreads) void pack_zero_desc_kernel(uint32_t* const* __restrict__ outs, int count)
{
    static_assert(kPackRowWords == 2 * 4 * kPackThreads, "two uint4 per thread");
    if ((int)blockIdx.x >= count) return;
    uint4* const row = reinterpret_cast<uint4*>(outs[blockIdx.x]);
    row[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    row[kPackThreads + threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ __launch_bounds__(kPackThreads) void pack_keyswitch_desc_kernel(
    const PackDesc* __restrict__ terms, int count, const uint32_t* __restrict__ key, int tiles, int slices)
{
    static_assert(kPackThreads % kPackTile == 0, "a thread stages one tile slot");
    __shared__ uint32_t rows[(kPackNumBase + 1) * kPackThreads];
    __shared__ __attribute__((aligned(16))) uint8_t dig[kPackIBlock * kPackT * kPackTile];
    const int tid = threadIdx.x;
    const int c = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int slice = blockIdx.y;
    const int t0 = (int)plan::pack_tile_first(tile, kPackTile);
    const int nt = plan::pack_tile_inputs(tile, kPackTile, count);
    const int i_begin = plan::pack_slice_begin(slice, slices, kLvl0N), i_end = plan::pack_slice_begin(slice + 1, slices, kLvl0N);

    uint32_t acc[kPackTile];
#pragma unroll
    for (int t = 0; t < kPackTile; t++) acc[t] = 0u;
    rows[tid] = 0u;
    uint32_t* const col = rows + tid;
    const uint32_t* kbase = key + c * kPackThreads + tid;
    const int ts = tid % kPackTile;                // the tile slot this thread stages
    const uint32_t* const staged = ts < nt ? terms[t0 + ts].in : nullptr;

    for (int ib = i_begin; ib < i_end; ib += kPackIBlock) {
        const int ni = min(kPackIBlock, i_end - ib);
        __syncthreads();                   // the digits of the previous block have been read
        for (int ii = tid / kPackTile; ii < ni; ii += kPackThreads / kPackTile) {
            const uint32_t a = staged ? staged[ib + ii] + kPackRound : 0u;
#pragma unroll
            for (int j = 0; j < kPackT; j++) dig[(ii * kPackT + j) * kPackTile + ts] = (uint8_t)((a >> (32 - kPackBasebit * (j + 1))) & kPackNumBase);
        }
        __syncthreads();
        for (int ii = 0; ii < ni; ii++) {
            const uint32_t* krow_i = kbase + (size_t)(ib + ii) * kPackT * kPackNumBase * kPackRowWords;
            for (int j = 0; j < kPackT; j++) {
                const uint32_t* krow = krow_i + (size_t)j * kPackNumBase * kPackRowWords;
                uint32_t v[kPackNumBase];
#pragma unroll
                for (int k = 0; k < kPackNumBase; k++) v[k] = krow[k * kPackRowWords];
#pragma unroll
                for (int k = 0; k < kPackNumBase; k++) col[(k + 1) * kPackThreads] = v[k];     // this thread's column only: no barrier
                const uint32_t* dg = (const uint32_t*)(dig + (ii * kPackT + j) * kPackTile);
#pragma unroll
                for (int q = 0; q < kPackTile / 4; q++) {
                    if (4 * q < nt) {              // uniform
                        const uint32_t w = dg[q];  // the same address in every lane: a broadcast
#pragma unroll
                        for (int b = 0; b < 4; b++) acc[4 * q + b] += col[((w >> (8 * b)) & 0xffu) * kPackThreads];
                    }
                }
            }
        }
    }
    const int e = c * kPackThreads + tid;          // row word: polynomial e / N, coefficient e % N
    const int poly = e / kN, k = e % kN;
    const bool holds_b = slice == 0 && e == kN;
#pragma unroll
    for (int t = 0; t < kPackTile; t++) {
        if (t >= nt) continue;
        const PackDesc d = terms[t0 + t];          // uniform: the same descriptor in every lane
        uint32_t val = 0u - acc[t];
        if (holds_b) val += d.in[kLvl0N];
        const int kk = k + d.pos;
        if (kk >= kN) val = 0u - val;
        atomicAdd(d.out + poly * kN + (kk & (kN - 1)), val);
    }
}

}  // namespace cufhe_amd
