// The lvl20 key switch for large launches (kept apart from kernels_lvl2.hip.h, whose hash stamps the profiled
// blind rotation in profiles/kernel_facts.json).
#pragma once
#include "kernels_lvl2.hip.h"
#include "ks_matrix.h"

namespace cufhe_amd {

// ----------------------------------------------------------------------------------
// The lvl20 key switch with the table shared through LDS: keyswitch_kernel (kernels.hip.h) over the lvl20 shape -- 2048 values
// a'_j of 64 bits per ciphertext, t = 7 digits each, 14 candidate rows of 640 words per j (35 KiB contiguous in the padded layout).
// A workgroup keeps the digit words of at most 1024 steps, so a launch always cuts j into at least two runs (KsDims::min_slices).
// L2 traffic drops 16x against keyswitch_direct_kernel<KsShapeLvl2, 1> (a workgroup per ciphertext, wave w takes a'_j for j in
// [128 w, 128 w + 128), rows straight from L2).
// ----------------------------------------------------------------------------------
struct KsShapeLvl2 {
    using Desc = LinDesc64;
    static constexpr int kn = k2N, t = k2KsT, row_pad = kKsRowPad, n_out = kLvl0N;
    // iksoffsetgen<lvl20> + roundoffset (include/keyswitch_gpu.cuh:13-23,92-98); only the top t*basebit = 14 bits carry digits
    static constexpr uint64_t koff()
    {
        uint64_t o = 1ull << (64 - (1 + k2KsBasebit * k2KsT));
        for (int i = 1; i <= k2KsT; i++) o += ((1ull << k2KsBasebit) / 2) << (64 - i * k2KsBasebit);
        return o;
    }
    static __device__ __forceinline__ uint32_t digit_word(const Desc& d, int j)
    {
        const uint64_t v = (uint64_t)(int64_t)d.ca * d.in0[j] + (uint64_t)(int64_t)d.cb * d.in1[j];
        return (uint32_t)((v + koff()) >> 48);
    }
    static __device__ __forceinline__ uint32_t bprime(const Desc& d)
    {
        const uint64_t v = (uint64_t)(int64_t)d.ca * d.in0[kn] + (uint64_t)(int64_t)d.cb * d.in1[kn];
        return (uint32_t)((v + d.off + (1ull << 31)) >> 32);           // rounding narrowing, :100-101
    }
};
static_assert(k2KsBasebit == kKsBasebit && k2KsNumBase == kKsNumBase, "keyswitch_kernel decodes digits of two bits");
static_assert(KsDims<KsShapeLvl2>::step_bytes == k2KsStepRows * kKsRowPad * 4 && KsDims<KsShapeLvl2>::min_slices == 2, "lvl20 shape");

// ----------------------------------------------------------------------------------
// The lvl10 key switch of a large launch as an exact int8 matrix product on the matrix cores (arithmetic: ks_matrix.h).
//   out[c][i] = b'_c [i = n] + sum_{j, kappa, v} coeff(c, j, kappa, v) * KSK[j][kappa][v][i]       coeff in {-1, 0, 1}
// is (count x 16384) . (16384 x 640 words); every key word is kept in four balanced base-256 digits (ks_mm_key_kernel, once per
// Initialize), so the product is four int8 planes with exact int32 sums (|sum| <= 2^21) that the epilogue adds with shifts:
// the same words as keyswitch_kernel.  One k-step of v_mfma_i32_32x32x32_i8 is two values of j: lane half h of a fragment holds
// the 16 rows (kappa, v) of j = 2 s + h, in the slot order of ksmm::slot_kappa / slot_v for A and B alike.
//   A  a wave expands the 16-bit digit words of its 64 ciphertexts (ks_mm_digits_kernel, once per launch) through a 256-entry
//      LDS table (digit byte -> 8 coefficients); A never goes through memory.
//   B  the matrix-form key [j][column < 2560][16] int8, column = (word block of 32, plane, word in the block): a lane's fragment is
//      one 16-byte piece, 32 lanes read 512 contiguous bytes, and the four planes of a word fall on the same lane of a wave's four
//      accumulator tiles.  Each wave requests its own pieces from L2 by LDS-DMA, kKsMmDepth k-steps ahead, and reads them back
//      from LDS; waves share nothing, so there is no barrier in the loop.
// A workgroup is ONE wave: a tile of kKsMmRows = 64 ciphertexts (two A fragments) x 32 words (four planes), 8 accumulator tiles
// of 16 registers, 8 MFMAs per 4 B pieces.  4096 ciphertexts are 64 x 20 = 1280 workgroups, five per CU in a single round (640 =
// 2^7 * 5 words: no tiling gives a multiple of 256 without the 5).  L2 traffic: the 42 MB key once per tile of 64 rows, 2.7 GB for
// 4096 ciphertexts, plus 0.16 GB of digit words; workgroups are numbered so that an XCD's L2 serves at most three word blocks.
// ----------------------------------------------------------------------------------
constexpr int kKsMmRows = 64;                 // ciphertexts per workgroup tile (two A fragments of 32 rows)
constexpr int kKsMmWords = 32;                // output words per workgroup tile (x 4 planes = four 32-column accumulator tiles)
constexpr int kKsMmWordBlocks = kKsRowPad / kKsMmWords;                      // 20
constexpr int kKsMmColumns = kKsRowPad * ksmm::kPlanes;                      // 2560 int8 columns
constexpr int kKsMmSteps = KsShapeDefault::kn / 2;                           // 512 MFMA k-steps of two j each
constexpr int kKsMmDepth = 6;                 // k-steps of B pieces and digit words in flight per wave
constexpr int kKsMmSlotBytes = ksmm::kPlanes * 1024 + 256;                   // one k-step in LDS: four B pieces of 1 KiB, the digit words
constexpr int kKsMmRequests = ksmm::kPlanes + 1;                             // LDS-DMA requests per k-step
static_assert((kKsMmDepth - 1) * kKsMmRequests < 64, "the requests in flight fit the wait counter");
static_assert(5 * (kKsMmDepth * kKsMmSlotBytes + 2048) <= 160 * 1024, "five workgroups per CU");
constexpr size_t kKsMmKeyBytes = (size_t)KsShapeDefault::kn * kKsMmColumns * ksmm::kSlots;     // 41 943 040
constexpr int kKsMmDigitChunk = 64;           // k-steps per workgroup of ks_mm_digits_kernel
static_assert(KsShapeDefault::t == ksmm::kFields && KsShapeDefault::t * kKsNumBase == ksmm::kSlots && KsShapeDefault::kn <= ksmm::kKnMax,
              "ks_matrix.h is written for the lvl10 shape");
static_assert(kKsMmSteps % 2 == 0 && kKsMmSteps % kKsMmDigitChunk == 0 && kKsRowPad % kKsMmWords == 0, "whole tiles");
// digit words of a launch: [tile][k-step][lane] u32, bits 0..15 row (lane & 31), bits 16..31 row 32 + (lane & 31), of j = 2 s + (lane >> 5)
inline size_t ks_mm_digit_bytes(size_t count) { return (count + kKsMmRows - 1) / kKsMmRows * kKsMmSteps * 64 * sizeof(uint32_t); }

// lds_dma16 (ntt_wave.h) for 4 bytes per lane: 256 bytes from `src_uniform + voff`, lane L lands at dst + 4 L
__device__ __forceinline__ void lds_dma4(const char* src_uniform, uint32_t voff, char* dst_uniform)
{
    const uint32_t base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)dst_uniform;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" ::"v"(voff), "s"(src_uniform), "s"(base) : "memory", "m0");
#pragma clang diagnostic pop
}

typedef int ksmm_v4i __attribute__((ext_vector_type(4)));
typedef int ksmm_v16i __attribute__((ext_vector_type(16)));

// The padded table [j][kappa][v - 1][640] u32 -> [j][column][16] int8 (grid: kn x kKsMmColumns / 256 workgroups of 256 threads)
__global__ __launch_bounds__(256) void ks_mm_key_kernel(const uint32_t* __restrict__ ksk_padded, ksmm_v4i* __restrict__ key_mm)
{
    const int j = blockIdx.x, col = blockIdx.y * 256 + threadIdx.x;
    const int wb = col / (kKsMmWords * ksmm::kPlanes), plane = col / kKsMmWords % ksmm::kPlanes, word = wb * kKsMmWords + col % kKsMmWords;
    uint32_t r[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < ksmm::kSlots; e++) {
        const int row = ksmm::slot_kappa(e) * kKsNumBase + (ksmm::slot_v(e) - 1);
        const uint32_t w = ksk_padded[((size_t)j * ksmm::kSlots + row) * kKsRowPad + word];
        r[e / 4] |= (uint32_t)(uint8_t)ksmm::plane_digit(w, plane) << (8 * (e % 4));
    }
    ksmm_v4i o;
    o.x = (int)r[0]; o.y = (int)r[1]; o.z = (int)r[2]; o.w = (int)r[3];
    key_mm[(size_t)j * kKsMmColumns + col] = o;
}

// The digit words S::digit_word(d, j) of a launch in the order the product kernel reads them; rows of the last tile beyond `count`
// get the word of all-zero coefficients.  Grid: tiles x kKsMmSteps / kKsMmDigitChunk workgroups of 256 threads.
template <class S>
__global__ __launch_bounds__(256) void ks_mm_digits_kernel(const typename S::Desc* __restrict__ descs, int count, uint32_t* __restrict__ dig)
{
    constexpr int J = 2 * kKsMmDigitChunk;           // values of j per workgroup
    __shared__ uint16_t dw[kKsMmRows][J + 2];
    const int tile = blockIdx.x, chunk = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int rr = wave; rr < kKsMmRows; rr += 4) {
        const int g = tile * kKsMmRows + rr;
        if (g < count) {
            const typename S::Desc d = descs[g];
            for (int jl = lane; jl < J; jl += 64) dw[rr][jl] = (uint16_t)S::digit_word(d, chunk * J + jl);
        } else {
            for (int jl = lane; jl < J; jl += 64) dw[rr][jl] = (uint16_t)ksmm::kNullDigitWord;
        }
    }
    __syncthreads();
    const int half = lane >> 5, r = lane & 31;
    for (int sl = wave; sl < kKsMmDigitChunk; sl += 4) {
        const uint32_t v = (uint32_t)dw[r][2 * sl + half] | (uint32_t)dw[r + 32][2 * sl + half] << 16;
        dig[((size_t)tile * kKsMmSteps + chunk * kKsMmDigitChunk + sl) * 64 + lane] = v;
    }
}

// two waves per SIMD (256 registers each, accumulators included): the five workgroups of a CU then run at once
template <class S>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void keyswitch_mm_kernel(
    const typename S::Desc* __restrict__ descs, int count, const ksmm_v4i* __restrict__ key_mm, const uint32_t* __restrict__ dig)
{
    __shared__ uint64_t tab[256];                    // digit byte -> the 8 coefficients of its four fields (two A registers)
    __shared__ __attribute__((aligned(16))) char ring[kKsMmDepth * kKsMmSlotBytes];
    const int lane = threadIdx.x, half = lane >> 5, n = lane & 31;
    const int tiles = (count + kKsMmRows - 1) / kKsMmRows, total = tiles * kKsMmWordBlocks;
    // workgroups i, i + 8, ... run on one XCD: give them consecutive tiles, word block major, so that its L2 holds few word blocks
    const int id = blockIdx.x;
    const int t = total % 8 == 0 ? (id % 8) * (total / 8) + id / 8 : id;
    const int wb = t / tiles, tile = t % tiles;
#pragma unroll
    for (int m = 0; m < 4; m++) tab[lane * 4 + m] = ksmm::expand_byte((unsigned)(lane * 4 + m));
    __syncthreads();

    // B: lane (n, half) of k-step s takes [j = 2 s + half][wb * 128 + plane * 32 + n]; digit words: [tile][s][lane].  Both come through
    // LDS by LDS-DMA (lds_dma16, ntt_wave.h: invisible to the compiler, which otherwise sinks every load of a register pipeline to
    // its use and waits out the L2 round trip eight times per k-step): a ring of kKsMmDepth k-steps per wave, five requests per
    // k-step (four 1 KiB pieces of B, 256 bytes of digit words), waited for by count.  A wave reads only what its own requests
    // wrote, so there is no barrier.
    const char* bbase = (const char*)key_mm + wb * (kKsMmWords * ksmm::kPlanes * ksmm::kSlots);
    const uint32_t bvoff = (uint32_t)(half * kKsMmColumns + n) * ksmm::kSlots;
    const char* dbase = (const char*)dig + (size_t)tile * kKsMmSteps * 256;
    auto issue = [&](int s, int slot) {              // past the last k-step: that one again, never read, so that the counts stay uniform
        const int sc = s < kKsMmSteps ? s : kKsMmSteps - 1;
        const char* src = bbase + (size_t)sc * (2 * kKsMmColumns * ksmm::kSlots);
        char* dst = ring + slot * kKsMmSlotBytes;
#pragma unroll
        for (int pl = 0; pl < ksmm::kPlanes; pl++) lds_dma16(src + pl * (kKsMmWords * ksmm::kSlots), bvoff, dst + pl * 1024);
        lds_dma4(dbase + sc * 256, (uint32_t)lane * 4, dst + ksmm::kPlanes * 1024);
    };
    struct Frag { ksmm_v4i b[ksmm::kPlanes], a0, a1; };
    auto expand = [&](uint32_t w16) {                // a 16-bit digit word -> the A fragment of its ciphertext and j
        const uint64_t hi = tab[(w16 >> 8) & 0xffu], lo = tab[w16 & 0xffu];
        ksmm_v4i a;
        a.x = (int)(uint32_t)hi; a.y = (int)(uint32_t)(hi >> 32); a.z = (int)(uint32_t)lo; a.w = (int)(uint32_t)(lo >> 32);
        return a;
    };
    auto read = [&](int slot, Frag& f) {
        const char* p = ring + slot * kKsMmSlotBytes;
#pragma unroll
        for (int pl = 0; pl < ksmm::kPlanes; pl++) f.b[pl] = *(const ksmm_v4i*)(p + pl * 1024 + lane * 16);
        const uint32_t w = *(const uint32_t*)(p + ksmm::kPlanes * 1024 + lane * 4);
        f.a0 = expand(w & 0xffffu);
        f.a1 = expand(w >> 16);
    };
#pragma unroll
    for (int i = 0; i < kKsMmDepth; i++) issue(i, i);

    ksmm_v16i acc[2][ksmm::kPlanes];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int pl = 0; pl < ksmm::kPlanes; pl++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[m][pl][i] = 0;

    Frag cur;
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((kKsMmDepth - 1) * kKsMmRequests) : "memory");      // k-step 0 has landed
    read(0, cur);
    int slot = 0;
#pragma unroll 2
    for (int s = 0; s < kKsMmSteps; s++) {
        const int nslot = slot + 1 == kKsMmDepth ? 0 : slot + 1;
        // k-step s + 1 has landed (requested so far: up to s + kKsMmDepth - 1), and the reads of k-step s, whose slot is requested
        // again below, have returned
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((kKsMmDepth - 2) * kKsMmRequests) : "memory");
        Frag nxt;
        read(nslot, nxt);                            // the fragments of k-step s + 1 travel while the MFMAs of s run
#pragma unroll
        for (int pl = 0; pl < ksmm::kPlanes; pl++) {
            acc[0][pl] = __builtin_amdgcn_mfma_i32_32x32x32_i8(cur.a0, cur.b[pl], acc[0][pl], 0, 0, 0);
            acc[1][pl] = __builtin_amdgcn_mfma_i32_32x32x32_i8(cur.a1, cur.b[pl], acc[1][pl], 0, 0, 0);
        }
        issue(s + kKsMmDepth, slot);
        cur = nxt;
        slot = nslot;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the requests past the end

    // C: register i of lane (n, half) is row 8 (i / 4) + 4 half + i % 4 of its 32-row fragment, column n; words above n_out are pad
    const int word = wb * kKsMmWords + n;
    if (word > S::n_out) return;
#pragma unroll
    for (int m = 0; m < 2; m++) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int g = tile * kKsMmRows + m * 32 + 8 * (i / 4) + 4 * half + i % 4;
            if (g >= count) continue;
            uint32_t v = ksmm::recombine(acc[m][0][i], acc[m][1][i], acc[m][2][i], acc[m][3][i]);
            if (word == S::n_out) v += S::bprime(descs[g]);
            descs[g].out[word] = v;                  // 4-byte aligned only (ciphertexts packed at n_out + 1 words)
        }
    }
}

}  // namespace cufhe_amd
