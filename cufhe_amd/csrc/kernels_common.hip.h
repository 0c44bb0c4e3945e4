// kernels_common.hip.h -- parameters, descriptor and LDS maps shared by the kernel files (kernels.hip.h and the
// separately compiled kernels_ll.hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ntt_wave.h"

namespace cufhe_amd {

// TFHE parameters.  Another set is NOT just a change of these lines: the
// static_asserts below tie l, Bgbit and N to the FP64 prime (exactness of the external product) and
// to the lazy-reduction schedule of ntt_wave.h; a set that fails them needs the limb split of
// kernels_lvl2.hip.h.
constexpr int kLvl0N = 630;            // lvl0param::n
constexpr int kNbit = 10;              // lvl1param::nbit
constexpr int kL = 3;                  // lvl1param::l
constexpr int kBgbit = 6;              // lvl1param::Bgbit
constexpr int kKsT = 8;                // lvl10param::t
constexpr int kKsBasebit = 2;          // lvl10param::basebit
constexpr uint32_t kMu = 1u << 29;     // lvl0/lvl1 mu
constexpr int kLvl0Words = kLvl0N + 1;
constexpr int kLvl1Words = kN + 1;
constexpr int kBkRows = 2 * kL;                         // (k+1) l
constexpr int kBkPolysPerStep = kBkRows * 2;            // (k+1)^2 l = 12
constexpr size_t kBkStepDoubles = (size_t)kBkPolysPerStep * kN;   // 12288 doubles = 98304 B
constexpr int kKsRowWords = kLvl0Words;                 // 631
constexpr int kKsNumBase = 1 << (kKsBasebit - 1);       // 2

// Exactness of the external product over the FP64 prime (fpfield.h): the true integer sum of one
// CMux output coefficient, |sum| <= (k+1) l N (Bg/2) 2^31 with the key read as signed words, must
// stay below p/2 or the centred lift returns a wrong torus word.
constexpr double kExtProdSumBound = 2.0 * kL * kN * (double)(1u << (kBgbit - 1)) * 2147483648.0;
static_assert(kExtProdSumBound < fpf::P / 2, "(k+1) l N (Bg/2) 2^31 >= p/2: this parameter set needs the limb split (kernels_lvl2.hip.h)");
// ... and of the lazy-reduction schedule: digits of magnitude Bg/2 through the forward transform,
// then (k+1) l unreduced wide products per accumulator
constexpr double kDigitSpectrumBound = forward_digit_spectrum_bound((double)(1u << (kBgbit - 1)));
static_assert(kDigitSpectrumBound > 0, "forward NTT of gadget digits: a stage input exceeds its multiplication's range");
static_assert(pointwise_sum_fits(kDigitSpectrumBound, kBkRows), "(k+1) l unreduced pointwise products exceed 2^53");
static_assert(kL * kBgbit <= 32 - 1, "decomposition wider than the torus word");

// out = ca * in0 + cb * in1 + (0, ..., 0, off): the linear part of every gate
struct LinDesc {
    const uint32_t* in0;
    const uint32_t* in1;   // never null (equal to in0 when cb == 0)
    uint32_t* out;
    int32_t ca, cb;
    uint32_t off;
    uint32_t pad;          // blind rotations: test vector, 0 = the constant mu, else row (pad & 0xff) - 1 of the device's user table and
                           // s = pad >> 8 (desc_shift): 2^s outputs of one rotation (multi-output user gates; 0 for every other rotation)
};

// User gates (cufhe_amd_define_gate): rows of kN torus words, one per definition, in every device's table
constexpr int kMaxUserGates = 64;

// Coefficient e of the initial accumulator's b polynomial, X^bbar * TV in Z[X]/(X^N + 1): TV[e - bbar] when 0 <= e - bbar < N, the
// negacyclic wrap with a sign otherwise.  tv == nullptr: TV = mu everywhere (RotatedTestVector, include/gatebootstrapping_gpu.cuh:29-52).
__device__ __forceinline__ uint32_t rotated_tv_coef(const uint32_t* __restrict__ tv, uint32_t bbar, uint32_t e)
{
    if (!tv) {
        const bool neg = (bbar != 2 * kN) && ((e < (bbar & (kN - 1))) != ((bbar >> kNbit) != 0));
        return neg ? 0u - kMu : kMu;
    }
    const uint32_t k = (e - bbar) & (2 * kN - 1);
    const uint32_t v = tv[k & (kN - 1)];
    return k >= (uint32_t)kN ? 0u - v : v;
}
// the row a rotation's descriptor selects in `tvs` ([kMaxUserGates][kN]), nullptr for the constant mu
__device__ __forceinline__ const uint32_t* desc_tv(const uint32_t* __restrict__ tvs, uint32_t pad)
{
    return pad ? tvs + (size_t)((pad & 0xffu) - 1) * kN : nullptr;
}

// Multi-output user gates (cufhe_amd_define_gate_multi, many-LUT bootstrapping): 2^s functions interleaved in one test vector, the
// modulus switch rounded to multiples of 2^s, outputs j = 0 .. 2^s - 1 extracted at index j of the one rotated accumulator.
constexpr int kMaxOutputShift = 3;                       // at most 8 outputs
__host__ __device__ constexpr uint32_t make_pad(int row, int s) { return (uint32_t)(row + 1) | ((uint32_t)s << 8); }
__device__ __forceinline__ int desc_shift(uint32_t pad) { return (int)(pad >> 8); }
// abar_i = ((a_i + 2^(30 - nbit + s)) >> (31 - nbit + s)) << s and bbar = 2N - ((b >> (31 - nbit + s)) << s); s = 0 is the gates' own
__device__ __forceinline__ uint32_t ms_abar(uint32_t a, int s) { return ((a + (1u << (32 - 2 - kNbit + s))) >> (32 - 1 - kNbit + s)) << s; }
__device__ __forceinline__ uint32_t ms_bbar(uint32_t b, int s) { return 2 * kN - ((b >> (32 - 1 - kNbit + s)) << s); }
// Coefficient e (a_e, b_e) of the rotated accumulator into outputs j = 1 .. nout - 1 (lvl1 TLWEs of kN + 1 words, contiguous behind
// output 0 at `out`): SampleExtract(j) is out_j[m] = a[j - m] (m <= j), -a[N + j - m] (m > j), out_j[N] = b[j].
__device__ __forceinline__ void extract_more(uint32_t* __restrict__ out, int nout, uint32_t e, uint32_t a, uint32_t b)
{
    for (int j = 1; j < nout; j++) {
        uint32_t* o = out + (size_t)j * (kN + 1);
        if (e <= (uint32_t)j) {
            o[j - e] = a;
            if (e == (uint32_t)j) o[kN] = b;
        } else {
            o[kN + j - e] = 0u - a;
        }
    }
}

// Device fault word (one uint32 per device in host-visible memory, DeviceState::fault): bits a kernel sets when it
// detects that its own result cannot be trusted.  The host turns any set bit into status -5 (capi.hip: device_fault).
constexpr uint32_t kFaultLl2SyncTimeout = 1u;      // blind_rotate_ll2_kernel: the inverse waves' LDS rendezvous timed out

// NTT-only kernels (key conversion, product check): 4 waves per workgroup
constexpr int kNttWavesPerBlock = 4;
constexpr int kNttThreads = 64 * kNttWavesPerBlock;
constexpr int kNttLdsBytes = kLdsTableBytes + kNttWavesPerBlock * kTileBytes;   // 49920

// Blind rotate: ONE 8-wave workgroup per CU (2 waves per SIMD).  Its LDS holds the twiddle
// tables, one transpose tile per wave, the abar list of every wave and three 16 KiB
// buffers for the TRGSW row shared by the 8 waves (the BK tile staged in LDS).
constexpr int kBrWavesPerBlock = 8;
constexpr int kBrThreads = 64 * kBrWavesPerBlock;                               // 512
constexpr int kBkRowBytes = 2 * kN * 8;                                         // 16384: one TRGSW row (2 polys)
constexpr int kAbarBytes = 1280;                                                // 630 x u16, padded
constexpr int kBkRowBuffers = 3;
// LDS map: [row buffers][twiddle tables][tiles][abar lists].  The row buffers come first so
// that "buffer + piece" offsets (< 64 KiB) fold into the DS instructions' offset field.
constexpr int kBrLdsBk = 0;
constexpr int kBrLdsTables = kBrLdsBk + kBkRowBuffers * kBkRowBytes;            // 49152
constexpr int kBrLdsTiles = kBrLdsTables + kLdsTablePackedBytes;                // the packed r4 tables (ntt_wave.h)
constexpr int kBrLdsAbar = kBrLdsTiles + kBrWavesPerBlock * kTileBytes;
constexpr int kBrLdsBytes = kBrLdsAbar + kBrWavesPerBlock * kAbarBytes;         // 145920

// gadget decomposition constants, include/gatebootstrapping_gpu.cuh:18-27,145-150
__host__ __device__ constexpr uint32_t decomp_offset()
{
    uint32_t o = 0;
    for (int i = 1; i <= kL; i++) o += (1u << (kBgbit - 1)) << (32 - i * kBgbit);
    return o + (1u << (32 - kL * kBgbit - 1));     // + roundoffset
}
// digit_d = field_d(t) - Bg/2 = sign-extended field_d(t ^ mask): flipping the top bit of each
// Bgbit-wide field adds Bg/2 modulo Bg without carrying into the next digit
__host__ __device__ constexpr uint32_t decomp_signmask()
{
    uint32_t m = 0;
    for (int i = 1; i <= kL; i++) m |= (1u << (kBgbit - 1)) << (32 - i * kBgbit);
    return m;
}

}  // namespace cufhe_amd
