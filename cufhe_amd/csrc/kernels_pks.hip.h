// kernels_pks.hip.h -- circuit bootstrapping (CGGI17 section 4, TFHEpp's CircuitBootstrapping): the device pieces after the lvl02
// rotations of kernels_lvl2*.hip.h.  A lvl0 TLWE becomes a lvl1 TRGSW [(k+1) l][k+1][N] (l = 3, Bgbit = 6) in three steps:
//   1. l blind rotations through the lvl2 ring with the constant test vectors mu_r = 2^(57 - 6 r) (RotDesc2::pad = 57 - 6 r), then
//      + mu_r on the b word (cb_add_mu_kernel): lvl2 TLWEs of bit * 2^(64 - 6 (r + 1));
//   2. private key switching lvl2 -> lvl1 of each of them under the two key functions f_0 = -s1(X), f_1 = 1
//      (private_keyswitch_kernel): TRGSW row c l + r = PrivKS_c(tlwe2_r);
//   3. TRGSW2NTT (bk_to_ntt_kernel, kernels.hip.h) where the caller wants the NTT domain.
#pragma once
#include "kernels_lvl2.hip.h"
#include "launch_plan.h"

namespace cufhe_amd {

constexpr int kCbL = 3;                    // lvl1 TRGSW of the output: l = 3, Bgbit = 6 (the rows of orc_bkgen)
constexpr int kCbBgbit = 6;
constexpr int kCbRowWords = 2 * kN;        // one TRLWE row: k + 1 = 2 polynomials of N = 1024
constexpr int kCbTrgswWords = 2 * kCbL * kCbRowWords;     // 12288 uint32: the layout cufhe_amd_trgsw_to_ntt_batch takes
static_assert(kCbTrgswWords == (int)kBkStepDoubles, "a circuit-bootstrapped TRGSW is one bootstrapping-key step");
// private key switching lvl2 -> lvl1 (TFHEpp lvl21param): t = 10 digits of basebit = 3 over the 2049 words of a lvl2 TLWE
constexpr int kPksT = 10;
constexpr int kPksBasebit = 3;
constexpr int kPksNumBase = (1 << kPksBasebit) - 1;       // 7 rows per (i, j): digit v = 1 .. 7
constexpr int kPksIn = k2N + 1;
constexpr size_t kPksKeyWordsPerU = (size_t)kPksIn * kPksT * kPksNumBase * kCbRowWords;
constexpr size_t kPksKeyWords = 2 * kPksKeyWordsPerU;     // 587 489 280 uint32 = 2.35 GB: K[u][i][j][v - 1][k + 1][N]
constexpr uint64_t kPksRound = 1ull << (64 - kPksT * kPksBasebit - 1);
static_assert(kPksT * kPksBasebit <= 32, "the digits must fit the 32-bit output torus");
constexpr uint32_t cb_mu_log2(int r) { return (uint32_t)(63 - (r + 1) * kCbBgbit); }   // RotDesc2::pad of rotation r: 57, 51, 45

// b + mu_r on every lvl2 TLWE of [count][l][N2 + 1]: the message becomes bit * 2^(64 - 6 (r + 1))
__global__ __launch_bounds__(256) void cb_add_mu_kernel(uint64_t* __restrict__ tlwe2, int n)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x < n) tlwe2[(size_t)x * kPksIn + k2N] += 1ull << cb_mu_log2(x % kCbL);
}

// The one-rotation form ("cb_rotations" 1): one rotation per input from the library's test-vector row (kCbRow2: TV[4 q + r] = mu_r,
// TV[4 q + 3] = 0) with output shift kCbShift = 2 leaves SampleExtract(0 .. 3) in all[count][4][N2 + 1]; row r < l of input g goes to
// tlwe2[g][r] with mu_r added to b.  One workgroup per row.
constexpr int kCbShift = 2;
static_assert((1 << kCbShift) > kCbL, "the rows of one TRGSW fit the outputs of one rotation");
__global__ __launch_bounds__(256) void cb_gather_mu_kernel(const uint64_t* __restrict__ all, uint64_t* __restrict__ tlwe2, int rows)
{
    const int x = blockIdx.x;
    if (x >= rows) return;
    const int g = x / kCbL, r = x % kCbL;
    const uint64_t* src = all + ((size_t)g * (1 << kCbShift) + r) * kPksIn;
    uint64_t* dst = tlwe2 + (size_t)x * kPksIn;
    for (int i = threadIdx.x; i < kPksIn; i += 256) dst[i] = src[i] + (i == k2N ? 1ull << cb_mu_log2(r) : 0ull);
}

// Private key switch.  Input x (a lvl2 TLWE) and key function u give the TRLWE
//     0 - sum_i sum_j [a_ij != 0] K_u[i][j][a_ij - 1],   a_ij = ((tlwe2[i] + 2^33) >> (64 - 3 (j + 1))) & 7,
// written to out + (x / L) (2 L) 2N + (u L + x % L) 2N (L = rows_per_out: 3 for a TRGSW, 1 for the stand-alone entry point).
// Workgroup = (key function u, chunk c of 256 of the 2N output words, tile of up to kPksTile inputs, slice of i); thread = one output
// word of every input of the tile, kept in registers.  For each (i, j) the thread loads its word of the 7 candidate rows once (one
// coalesced sweep of the key slice per tile) into its own column of LDS, row 0 = 0, and every input of the tile adds the row its digit
// picks: the digit is the same for all lanes, so the LDS reads are conflict-free and nothing branches.  Slices of i (small batches:
// the key sweep spread over the chip) add their partial sums with vector atomics into a zeroed output; uint32 wrap-around addition is
// order-independent, so the words are the same for every shape.
constexpr int kPksThreads = 256;
constexpr int kPksTile = 64;
constexpr int kPksIBlock = 16;             // input words whose digits are staged per pass
constexpr int kPksChunks = kCbRowWords / kPksThreads;     // 8
// The launch shape is plan::plan_private_keyswitch over this geometry.  The kernel cuts i inline, per = ceil(in / slices) without the
// clamp of plan::pack_slice_begin (its text and code stay as measured: profiles/r28_table_sum_body.md); the two cuts give every slice
// of every slice count the rule can return the same words
constexpr plan::PksGeometry kPksGeometry{kPksTile, kPksChunks, kPksIn, kPksIBlock};
static_assert(plan::slices_match_unclamped_cut(kPksIn, plan::pack_max_slices(kPksGeometry)), "the kernel's cut of i is plan::pack_slice_begin's");
__global__ __launch_bounds__(kPksThreads) void private_keyswitch_kernel(
    const uint64_t* __restrict__ in, int count, const uint32_t* __restrict__ key, uint32_t* __restrict__ out, int rows_per_out,
    int tiles, int slices)
{
    __shared__ uint32_t rows[(kPksNumBase + 1) * kPksThreads];
    __shared__ __attribute__((aligned(16))) uint8_t dig[kPksIBlock * kPksT * kPksTile];
    const int tid = threadIdx.x;
    const int uc = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int u = uc / kPksChunks, c = uc % kPksChunks;
    const int slice = blockIdx.y;
    const int t0 = tile * kPksTile;
    const int nt = min(kPksTile, count - t0);
    const int per = (kPksIn + slices - 1) / slices;
    const int i_begin = slice * per, i_end = min(kPksIn, i_begin + per);

    uint32_t acc[kPksTile];
#pragma unroll
    for (int t = 0; t < kPksTile; t++) acc[t] = 0u;
    rows[tid] = 0u;
    uint32_t* const col = rows + tid;
    const uint32_t* kbase = key + (size_t)u * kPksKeyWordsPerU + c * kPksThreads + tid;

    for (int ib = i_begin; ib < i_end; ib += kPksIBlock) {
        const int ni = min(kPksIBlock, i_end - ib);
        __syncthreads();                   // the digits of the previous block have been read
        for (int e = tid; e < ni * kPksTile; e += kPksThreads) {
            const int ii = e / kPksTile, t = e % kPksTile;
            const uint64_t a = t < nt ? in[(size_t)(t0 + t) * kPksIn + ib + ii] + kPksRound : 0ull;
#pragma unroll
            for (int j = 0; j < kPksT; j++) dig[(ii * kPksT + j) * kPksTile + t] = (uint8_t)((a >> (64 - kPksBasebit * (j + 1))) & kPksNumBase);
        }
        __syncthreads();
        for (int ii = 0; ii < ni; ii++) {
            const uint32_t* krow_i = kbase + (size_t)(ib + ii) * kPksT * kPksNumBase * kCbRowWords;
            for (int j = 0; j < kPksT; j++) {
                const uint32_t* krow = krow_i + (size_t)j * kPksNumBase * kCbRowWords;
                uint32_t v[kPksNumBase];
#pragma unroll
                for (int k = 0; k < kPksNumBase; k++) v[k] = krow[k * kCbRowWords];
#pragma unroll
                for (int k = 0; k < kPksNumBase; k++) col[(k + 1) * kPksThreads] = v[k];     // this thread's column only: no barrier
                const uint32_t* dg = (const uint32_t*)(dig + (ii * kPksT + j) * kPksTile);
#pragma unroll
                for (int q = 0; q < kPksTile / 4; q++) {
                    if (4 * q < nt) {              // uniform
                        const uint32_t w = dg[q];  // the same address in every lane: a broadcast
#pragma unroll
                        for (int b = 0; b < 4; b++) acc[4 * q + b] += col[((w >> (8 * b)) & 0xffu) * kPksThreads];
                    }
                }
            }
        }
    }
    const bool atomic = slices > 1;
#pragma unroll
    for (int t = 0; t < kPksTile; t++) {
        if (t >= nt) continue;
        const int x = t0 + t;
        uint32_t* o = out + (size_t)(x / rows_per_out) * (2 * rows_per_out) * kCbRowWords +
                      (size_t)(u * rows_per_out + x % rows_per_out) * kCbRowWords + c * kPksThreads + tid;
        if (atomic) atomicAdd(o, 0u - acc[t]);
        else *o = 0u - acc[t];
    }
}

}  // namespace cufhe_amd
