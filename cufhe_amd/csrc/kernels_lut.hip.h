// kernels_lut.hip.h -- the keyless helper of the encrypted-table lookup:
//
//   trlwe_spread_kernel    Spread(c) = X^(-stride floor(reps/2)) sum_{i < reps} X^(i stride) c on both polynomials of a TRLWE
//
// (the lookup's rotations are blind_rotate_wave<true> / ll_rotate<true> / ll2_rotate<true>, kernels.hip.h and kernels_ll.hip.h).
#pragma once
#include "kernels_common.hip.h"

namespace cufhe_amd {

// With chat[m] = c[m mod N] (-1)^floor(m / N), the negacyclic extension of one polynomial, coefficient k of Spread(c) is the window
//     W[m] = sum_{i < reps} chat[m - i stride]        at m = k + stride floor(reps/2),        W[m + N] = -W[m],
// a sum over one residue class mod stride.  The coefficients are therefore taken in CLASS-MAJOR order -- class rho = m mod stride after
// class rho - 1, each by rising m: the first N mod stride classes have floor(N / stride) + 1 members, the others floor(N / stride) -- and
// ONE ordinary prefix sum Q over that order serves every class: two members of a class are neighbours runs apart, so a run of a class
// is a difference of two values of Q.  For 0 <= m < N, t = floor(m / stride), R = reps stride <= N:
//     m - R >= 0     W[m] = Q(m) - Q(m - R)
//     m - R <  0     the t + 1 members of the class down to rho, minus (chat = -c there) the reps - 1 - t top members of the class of
//                    m + N:   W[m] = (Q(m) - Q(before the class)) - (Q(jmax) - Q(m - R + N)),   jmax = N - stride + rho
// One wavefront per polynomial; a lane loads and stores coefficients lane + 64 r (trlwe_rotate_kernel's mapping, coalesced) and scans the
// 16 consecutive positions 16 lane + r of the class-major order: a serial sum in registers, a wave scan of the 64 lane totals, and the
// prefix array left in LDS (pre[q + 1] = Q at position q, pre[0] = 0) for the gathers of the windows.  No loop is `reps` long; all
// arithmetic is uint32.  out must not overlap in (the host refuses it): other waves may still be loading.
constexpr int kSpreadWavesPerBlock = 4;
__global__ __launch_bounds__(64 * kSpreadWavesPerBlock) void trlwe_spread_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ in,
                                                                                 int polys, int stride, int reps)
{
    __shared__ uint32_t coef[kSpreadWavesPerBlock][kN];
    __shared__ uint32_t pre[kSpreadWavesPerBlock][kN + 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int poly = blockIdx.x * kSpreadWavesPerBlock + wave;
    const bool live = poly < polys;
    const uint32_t* p = in + (size_t)(live ? poly : 0) * kN;
#pragma unroll
    for (int r = 0; r < kRegs; r++) coef[wave][lane + 64 * r] = live ? p[lane + 64 * r] : 0u;
    __syncthreads();

    const int len = kN / stride, big = kN - len * stride;      // classes rho < big have len + 1 members
    const int split = big * (len + 1);                          // first position of the classes of len members
    auto class_start = [&](int rho) { return rho < big ? rho * (len + 1) : split + (rho - big) * len; };
    uint32_t v[kRegs], run = 0;
#pragma unroll
    for (int r = 0; r < kRegs; r++) {
        const int q = 16 * lane + r;
        const int rho = q < split ? q / (len + 1) : big + (q - split) / len;
        const int t = q - class_start(rho);
        run += coef[wave][rho + t * stride];
        v[r] = run;
    }
    uint32_t incl = run;                                        // inclusive wave scan of the lane totals
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    const uint32_t carry = incl - run;
    if (lane == 0) pre[wave][0] = 0u;
#pragma unroll
    for (int r = 0; r < kRegs; r++) pre[wave][16 * lane + r + 1] = carry + v[r];
    __syncthreads();
    if (!live) return;

    const int shift = stride * (reps / 2);
    uint32_t* o = out + (size_t)poly * kN;
#pragma unroll
    for (int r = 0; r < kRegs; r++) {
        const int k = lane + 64 * r;
        const bool neg = k + shift >= kN;
        const int m = neg ? k + shift - kN : k + shift;
        const int t = m / stride, rho = m - t * stride;
        const int start = class_start(rho), q = start + t;
        uint32_t w = pre[wave][q + 1];
        if (t >= reps) {
            w -= pre[wave][q + 1 - reps];
        } else {
            w -= pre[wave][start];
            const int jmax = kN - stride + rho;                 // the top member of the class of m + N
            const int tj = jmax / stride;
            const int qj = class_start(jmax - tj * stride) + tj;
            w -= pre[wave][qj + 1] - pre[wave][qj + 1 - (reps - 1 - t)];
        }
        o[k] = neg ? 0u - w : w;
    }
}

}  // namespace cufhe_amd
