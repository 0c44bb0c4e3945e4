// ks_matrix.h -- the arithmetic of the key switch written as an exact int8 matrix product (keyswitch_mm_kernel,
// kernels_ks2.hip.h).  Host only, standard library only: the device kernels call these functions and
// tests/host/ks_matrix.cpp checks them on the CPU (tests/test_ks_matrix.py).
//
// out[c][i] = b'_c [i = n] + sum over (j, kappa) of c1 * KSK[j][kappa][0][i] + c2 * KSK[j][kappa][1][i]   (mod 2^32)
// with (c1, c2) chosen by the 2-bit digit field f of a'_j (ks_digit_load / ks_digit_acc, kernels.hip.h).  Every key word is
// written once in four balanced base-256 digits, so the sum is four int8 x int8 -> int32 products that are put together again
// by shifts: sums mod 2^32 are order-free, so the words are those of keyswitch_kernel.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KSMM_HD __host__ __device__
#else
#define KSMM_HD
#endif

namespace ksmm {

constexpr int kPlanes = 4;         // balanced base-256 digits of a 32-bit word
constexpr int kFields = 8;         // 2-bit digit fields of one a'_j (t)
constexpr int kSlots = 16;         // rows of the key per j: kappa * 2 + (v - 1); also the k slots of one j in a fragment
constexpr int kKnMax = 1024;       // values a'_j per ciphertext

// slot e of a lane's 16-byte fragment (A and B alike) carries row (kappa, v) of the lane half's j: ONE function for both operands
KSMM_HD constexpr int slot_kappa(int e) { return e >> 1; }
KSMM_HD constexpr int slot_v(int e) { return (e & 1) + 1; }

// the coefficient of row v (1 or 2) under digit field f: f = 0: +row(v=2), 1: +row(v=1), 2: nothing, 3: -row(v=1)
KSMM_HD constexpr int coeff(unsigned f, int v) { return v == 2 ? (f == 0 ? 1 : 0) : (f == 1 ? 1 : f == 3 ? -1 : 0); }
// field kappa of a 16-bit digit word: most significant digit first (ks_field, kernels.hip.h)
KSMM_HD constexpr unsigned field(unsigned dw, int kappa) { return (dw >> (16 - 2 * (kappa + 1))) & 3u; }
// the coefficient in slot e of the fragment of digit word dw
KSMM_HD constexpr int slot_coeff(unsigned dw, int e) { return coeff(field(dw, slot_kappa(e)), slot_v(e)); }
// the digit word whose every coefficient is zero (rows of a tile beyond the launch)
constexpr unsigned kNullDigitWord = 0xAAAAu;

// Slots 8 q .. 8 q + 7 (fields 4 q .. 4 q + 3, one byte of the digit word) as the two 32-bit registers of an A fragment, slot e in
// byte e % 4 of register e / 4: what the kernel keeps in a 256-entry table
KSMM_HD constexpr uint64_t expand_byte(unsigned byte)
{
    uint64_t r = 0;
    for (int e = 0; e < 8; e++) r |= (uint64_t)(uint8_t)(int8_t)coeff((byte >> (6 - 2 * (e >> 1))) & 3u, slot_v(e)) << (8 * e);
    return r;
}

// balanced base-256 digit b of w: w = sum_b d_b 256^b (mod 2^32), d_b in [-128, 127], the carry out of the top digit dropped
KSMM_HD constexpr int plane_digit(uint32_t w, int b)
{
    int d = 0;
    for (int i = 0; i <= b; i++) {
        d = (int)(int8_t)(uint8_t)(w & 0xffu);
        w = (w >> 8) + (d < 0 ? 1u : 0u);        // (w - d) / 256
    }
    return d;
}
// the word of four plane sums (each an exact int32)
KSMM_HD constexpr uint32_t recombine(int32_t c0, int32_t c1, int32_t c2, int32_t c3)
{
    return (uint32_t)c0 + ((uint32_t)c1 << 8) + ((uint32_t)c2 << 16) + ((uint32_t)c3 << 24);
}

// a plane sum has at most one non-zero coefficient per (j, kappa) -- c1 and c2 are never both set -- and |d| <= 128
constexpr long long kMaxPartialSum = (long long)kKnMax * kFields * 2 * 128;      // both rows counted: 2^21
static_assert(kMaxPartialSum == (1ll << 21) && kMaxPartialSum < (1ll << 31), "plane sums are exact in int32");

}  // namespace ksmm
