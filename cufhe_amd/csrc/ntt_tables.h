// ntt_tables.h -- the twiddle tables of every transform: their layouts, which the device headers share, and the exact
// host arithmetic that fills them.  Host-only and free of HIP: plain g++ compiles it, and tests/host/ntt_tables_harness.cpp
// (tests/test_ntt_tables.py) checks every table on the CPU, byte for byte and property by property.
//
// All tables are cut from one kind of array: root[i] = psi^bitrev(i) (the reference's table order,
// src/ntt_gpu/ntt_gpuntt.cu:88-111), root[m + g] being the twiddle of group g at the stage with m groups, as a balanced
// residue in a double.  After the first log2(parts) stages a transform falls into `parts` independent sub-transforms
// (ntt_wave512.h) whose root arrays are selections of the full one.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "fpfield.h"

namespace cufhe_amd {

// ---- layouts ----
constexpr int kN = 1024;
constexpr int kTbCount = 15;         // per-lane twiddles of stages 4-7
constexpr int kTcCount = 12;         // per-lane twiddles of stages 8-9
constexpr int kTbpStride = 18;       // doubles per lambda in the packed stage 4-7 table (15 used)
constexpr int kTcpStride = 14;       // doubles per lane in the packed stage 8-9 table (12 used)

// tables of one 1024-point transform (ntt_wave.h)
struct NttTables {
    double tu_fwd[16];               // [k] k<15: root[2^lvl + j], lvl=floor(log2(k+1)), j=k+1-2^lvl
    double tu_inv[16];
    double tb_fwd[kTbCount * 16];    // [k][lambda]: root[16*2^lvl + lambda*2^lvl + j]
    double tb_inv[kTbCount * 16];
    double tc_fwd[kTcCount * 64];    // [k][lane]: k<4: root[256 + (lambda<<4|h<<2|k)]; else root[512 + (lambda<<5|h<<3|(k-4))]
    double tc_inv[kTcCount * 64];
    // The same per-lane twiddles PACKED per lane (filled for the r4 tables only): a lane's fifteen stage 4-7 twiddles and its
    // twelve stage 8-9 twiddles are contiguous, so a transform fetches them with 8 + 6 ds_read_b128 instead of 27 ds_read_b64
    // (the compiler pairs those into ds_read2_b64, which moves 128 B per LDS clock where ds_read_b128 moves 256).  The strides
    // -- 18 doubles = 144 bytes per lambda, 14 doubles = 112 bytes per lane -- put the sixteen lanes of every ds_read_b128 lane
    // group on sixteen different 4-bank slots.  [tbp_fwd | tbp_inv | tcp_fwd | tcp_inv] is one contiguous block.
    double tbp_fwd[16 * kTbpStride];
    double tbp_inv[16 * kTbpStride];
    double tcp_fwd[64 * kTcpStride];
    double tcp_inv[64 * kTcpStride];
};
constexpr int kLdsTablePackedDoubles = 2 * 16 * kTbpStride + 2 * 64 * kTcpStride;   // 2368
constexpr int kLdsTablePackedBytes = kLdsTablePackedDoubles * 8;                     // 18944
constexpr int kLdsTableDoubles = 2 * kTbCount * 16 + 2 * kTcCount * 64;   // 2016
constexpr int kLdsTableBytes = kLdsTableDoubles * 8;                        // 16128

constexpr int kH = 512;               // points of a half transform

// tables of ONE 512-point transform (ntt_wave512.h): a half of the 1024-point one, a quarter of the 2048-point one, or stand-alone
struct Ntt512Tables {
    double tu_fwd[8];                 // [k] k<7: root_h[2^lvl + j], lvl = floor(log2(k+1)), j = k+1-2^lvl
    double tu_inv[8];
    double tb_fwd[7 * 8];             // [k][lam]: root_h[8*2^lvl + lam*2^lvl + j]
    double tb_inv[7 * 8];
    double tc_fwd[7 * 64];            // [k][lane]: root_h[64*2^lvl + mu*2^lvl + j], mu = 8 lam + kap
    double tc_inv[7 * 64];
    // radix-4 form (ntt_wave512.h: q4): the product of a block's stage-a and first stage-b twiddle, u w (forward) / v w (inverse), per lam
    // and per lane; the wave-uniform block's sits in the spare slot 7 of tu_fwd / tu_inv.  Contiguous, in this order.
    double uwb_fwd[8], uwb_inv[8];
    double uwc_fwd[64], uwc_inv[64];
};
static_assert(sizeof(Ntt512Tables) == (16 + 1008 + 144) * 8, "Ntt512Tables: [tu 16 | tb, tc 1008 | radix-4 products 144] doubles");
constexpr int kLds512TableDoubles = 2 * 7 * 8 + 2 * 7 * 64;     // tb_fwd .. tc_inv, contiguous: 1008
constexpr int kLds512TableBytes = kLds512TableDoubles * 8;      // 8064 per half

// ---- exact arithmetic mod p ----
constexpr uint64_t mulmod_u64(uint64_t a, uint64_t b) { return (uint64_t)((unsigned __int128)a * b % fpf::P_U64); }
constexpr uint64_t powmod_u64(uint64_t a, uint64_t e)
{
    uint64_t r = 1;
    while (e) {
        if (e & 1) r = mulmod_u64(r, a);
        a = mulmod_u64(a, a);
        e >>= 1;
    }
    return r;
}
inline double balanced(uint64_t v) { return v > fpf::P_U64 / 2 ? -(double)(fpf::P_U64 - v) : (double)v; }
inline uint32_t bitrev(uint32_t x, int bits)
{
    uint32_t r = 0;
    for (int i = 0; i < bits; i++) r |= ((x >> i) & 1u) << (bits - 1 - i);
    return r;
}
// exact product mod p of two balanced residues held in doubles, balanced again
inline double mul_balanced(double a, double b)
{
    const uint64_t ua = a < 0 ? fpf::P_U64 - (uint64_t)(-a) : (uint64_t)a, ub = b < 0 ? fpf::P_U64 - (uint64_t)(-b) : (uint64_t)b;
    return balanced(mulmod_u64(ua, ub));
}
// N^-1, the factor the key transforms fold into the key
inline double n_inverse(int N) { return balanced(powmod_u64((uint64_t)N, fpf::P_U64 - 2)); }

// the 4096-th root of the N = 2048 ring
constexpr uint64_t kPsi4096 = 245080461804091ull;
static_assert(mulmod_u64(kPsi4096, kPsi4096) == fpf::PSI_2048 && (double)powmod_u64(kPsi4096, 1024) == fpf::ROOT4, "kPsi4096: psi^2 = PSI_2048, psi^1024 = I");

// ---- root arrays ----
struct Roots { std::vector<double> fwd, inv; };     // [m + g]; inv[i] = fwd[i]^-1; [0] is not a twiddle

// the 2^bits-point negacyclic transform whose 2^(bits+1)-th root of unity is psi
inline Roots negacyclic_roots(uint64_t psi, int bits)
{
    const uint32_t n = 1u << bits;
    const uint64_t psi_inv = powmod_u64(psi, fpf::P_U64 - 2);
    Roots r{std::vector<double>(n), std::vector<double>(n)};
    for (uint32_t i = 0; i < n; i++) {
        r.fwd[i] = balanced(powmod_u64(psi, bitrev(i, bits)));
        r.inv[i] = balanced(powmod_u64(psi_inv, bitrev(i, bits)));
    }
    return r;
}
// sub-transform h of `parts` (2: halves, 4: quarters): root_h[m + g] = root[parts m + h m + g]
inline Roots sub_transform(const Roots& r, int parts, int h)
{
    const size_t n = r.fwd.size() / parts;
    Roots s{std::vector<double>(n, 0.0), std::vector<double>(n, 0.0)};
    for (size_t m = 1; m < n; m <<= 1)
        for (size_t g = 0; g < m; g++) {
            s.fwd[m + g] = r.fwd[parts * m + h * m + g];
            s.inv[m + g] = r.inv[parts * m + h * m + g];
        }
    return s;
}

// A block of consecutive stages keeps its twiddles in heap order: slot k is twiddle j = k + 1 - 2^lvl of the block's stage
// lvl = floor(log2(k + 1)).  Its index in the root array when the block's first stage has `base` groups and this is group `lam` of them:
inline int block_index(int base, int lam, int k)
{
    int lvl = 0;
    while ((2 << lvl) <= k + 1) lvl++;
    return (base << lvl) + (lam << lvl) + k + 1 - (1 << lvl);
}

// ---- 1024-point tables ----
// r4: the tables of the radix-4 passes (ntt_r4.h).  A 16-register block uses the twiddles [w | u, I u | w_0..w_3 | u_0, I u_0, ..];
// the radix-4 butterfly never multiplies by the second twiddle of a fine pair (root[2m + 1] = I root[2m], -I for the inverse)
// but by the product of the first with the coarse twiddle: slot 2 = u w, slot 8 + 2g = u_g w_g (tc: slot 5 + 2g = u_g w_g).
inline void to_r4_block(double* t, int stride)       // t[k * stride], k < 15: one block of four stages
{
    t[2 * stride] = mul_balanced(t[1 * stride], t[0]);
    for (int g = 0; g < 4; g++) t[(8 + 2 * g) * stride] = mul_balanced(t[(7 + 2 * g) * stride], t[(3 + g) * stride]);
}
// one direction (forward or inverse) of an NttTables from its root array
inline void fill_direction(double* tu, double* tb, double* tc, double* tbp, double* tcp, const std::vector<double>& root, bool r4)
{
    for (int k = 0; k < 15; k++) {
        tu[k] = root[block_index(1, 0, k)];
        for (int lam = 0; lam < 16; lam++) tb[k * 16 + lam] = root[block_index(16, lam, k)];
    }
    for (int k = 0; k < kTcCount; k++)
        for (int lane = 0; lane < 64; lane++) {
            const int lam = lane & 15, h = lane >> 4;
            tc[k * 64 + lane] = root[k < 4 ? 256 + ((lam << 4) | (h << 2) | k) : 512 + ((lam << 5) | (h << 3) | (k - 4))];
        }
    if (!r4) return;
    to_r4_block(tu, 1);
    for (int lam = 0; lam < 16; lam++) to_r4_block(tb + lam, 16);
    for (int lane = 0; lane < 64; lane++)
        for (int g = 0; g < 4; g++) tc[(5 + 2 * g) * 64 + lane] = mul_balanced(tc[(4 + 2 * g) * 64 + lane], tc[g * 64 + lane]);
    // packed per lane (NttTables::tbp_fwd ..)
    for (int lam = 0; lam < 16; lam++)
        for (int k = 0; k < kTbCount; k++) tbp[lam * kTbpStride + k] = tb[k * 16 + lam];
    for (int lane = 0; lane < 64; lane++)
        for (int k = 0; k < kTcCount; k++) tcp[lane * kTcpStride + k] = tc[k * 64 + lane];
}
inline void fill_tables(NttTables& t, const Roots& root, bool r4 = false)
{
    memset(&t, 0, sizeof(t));
    fill_direction(t.tu_fwd, t.tb_fwd, t.tc_fwd, t.tbp_fwd, t.tcp_fwd, root.fwd, r4);
    fill_direction(t.tu_inv, t.tb_inv, t.tc_inv, t.tbp_inv, t.tcp_inv, root.inv, r4);
}

// ---- 512-point tables ----
inline void fill_direction_512(double* tu, double* tb, double* tc, const std::vector<double>& root)
{
    for (int k = 0; k < 7; k++) {
        tu[k] = root[block_index(1, 0, k)];
        for (int lam = 0; lam < 8; lam++) tb[k * 8 + lam] = root[block_index(8, lam, k)];
        for (int lane = 0; lane < 64; lane++) tc[k * 64 + lane] = root[block_index(64, 8 * (lane & 7) + (lane >> 3), k)];
    }
}
inline void fill_tables_512(Ntt512Tables& t, const Roots& root)
{
    memset(&t, 0, sizeof(t));
    fill_direction_512(t.tu_fwd, t.tb_fwd, t.tc_fwd, root.fwd);
    fill_direction_512(t.tu_inv, t.tb_inv, t.tc_inv, root.inv);
}
// Radix-4 form of a 512-point transform (ntt_wave512.h: q4): the product of a block's stage-a and first stage-b twiddle, u w
// (forward) and v w (inverse) -- in the spare slot 7 of tu_fwd / tu_inv for the wave-uniform block, in uwb_* / uwc_* per lam and per
// lane.  The second stage-b twiddle must be I times (forward) / -I times (inverse) the first: false if it is not.  For the halves
// and the quarters only: the kernels of the stand-alone transform run the radix-2 form.
inline bool r4_products_512(double* tu, const double* tb, const double* tc, double* uwb, double* uwc, double i4)
{
    if (mul_balanced(tu[1], i4) != tu[2]) return false;
    tu[7] = mul_balanced(tu[0], tu[1]);
    for (int lam = 0; lam < 8; lam++) {
        if (mul_balanced(tb[8 + lam], i4) != tb[16 + lam]) return false;
        uwb[lam] = mul_balanced(tb[lam], tb[8 + lam]);
    }
    for (int lane = 0; lane < 64; lane++) {
        if (mul_balanced(tc[64 + lane], i4) != tc[128 + lane]) return false;
        uwc[lane] = mul_balanced(tc[lane], tc[64 + lane]);
    }
    return true;
}
inline bool fill_r4_products_512(Ntt512Tables& t)
{
    return r4_products_512(t.tu_fwd, t.tb_fwd, t.tc_fwd, t.uwb_fwd, t.uwc_fwd, fpf::ROOT4) &&
           r4_products_512(t.tu_inv, t.tb_inv, t.tc_inv, t.uwb_inv, t.uwc_inv, -fpf::ROOT4);
}

// ---- the tables of the library ----
// the 1024-point transform, psi = PSI_2048
inline void build_tables(NttTables& t, bool r4 = false) { fill_tables(t, negacyclic_roots(fpf::PSI_2048, 10), r4); }
// t[0], t[1]: the two 512-point halves of the 1024-point transform; t[2]: the stand-alone 512-point negacyclic transform
// (psi_1024 = psi_2048^2)
inline void build_tables_512(Ntt512Tables (&t)[3])
{
    const Roots full = negacyclic_roots(fpf::PSI_2048, 10);
    for (int h = 0; h < 2; h++) fill_tables_512(t[h], sub_transform(full, 2, h));
    fill_tables_512(t[2], negacyclic_roots(mulmod_u64(fpf::PSI_2048, fpf::PSI_2048), 9));
}
// the two 1024-point halves of the 2048-point transform (kernels_lvl2.hip.h)
inline void build_tables_lvl2(NttTables (&t)[2])
{
    const Roots full = negacyclic_roots(kPsi4096, 11);
    for (int h = 0; h < 2; h++) fill_tables(t[h], sub_transform(full, 2, h));
}
// its four 512-point quarters (kernels_lvl2q.hip.h)
inline void build_tables_lvl2q(Ntt512Tables (&t)[4])
{
    const Roots full = negacyclic_roots(kPsi4096, 11);
    for (int q = 0; q < 4; q++) fill_tables_512(t[q], sub_transform(full, 4, q));
}

}  // namespace cufhe_amd
