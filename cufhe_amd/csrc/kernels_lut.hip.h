// kernels_lut.hip.h -- the keyless helper of the encrypted-table lookup:
//
//   trlwe_spread_kernel       Spread(c) = X^(-stride floor(reps/2)) sum_{i < reps} X^(i stride) c on both polynomials of a TRLWE
//   trlwe_spread_desc_kernel  the same from descriptors: scattered buffers, a (stride, reps) of its own per TRLWE (the recorded form)
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
// The work of one wavefront on one polynomial: `coef` and `pre` are the wave's rows of the workgroup's LDS arrays, p / o the polynomial
// read and written (ignored when !live: the wave then only keeps the workgroup's barriers).  stride and reps must be wave-uniform.
__device__ __forceinline__ void trlwe_spread_wave(uint32_t* __restrict__ o, const uint32_t* __restrict__ p, bool live, int stride, int reps,
                                                  uint32_t* __restrict__ coef, uint32_t* __restrict__ pre, int lane)
{
#pragma unroll
    for (int r = 0; r < kRegs; r++) coef[lane + 64 * r] = live ? p[lane + 64 * r] : 0u;
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
        run += coef[rho + t * stride];
        v[r] = run;
    }
    uint32_t incl = run;                                        // inclusive wave scan of the lane totals
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    const uint32_t carry = incl - run;
    if (lane == 0) pre[0] = 0u;
#pragma unroll
    for (int r = 0; r < kRegs; r++) pre[16 * lane + r + 1] = carry + v[r];
    __syncthreads();
    if (!live) return;

    const int shift = stride * (reps / 2);
#pragma unroll
    for (int r = 0; r < kRegs; r++) {
        const int k = lane + 64 * r;
        const bool neg = k + shift >= kN;
        const int m = neg ? k + shift - kN : k + shift;
        const int t = m / stride, rho = m - t * stride;
        const int start = class_start(rho), q = start + t;
        uint32_t w = pre[q + 1];
        if (t >= reps) {
            w -= pre[q + 1 - reps];
        } else {
            w -= pre[start];
            const int jmax = kN - stride + rho;                 // the top member of the class of m + N
            const int tj = jmax / stride;
            const int qj = class_start(jmax - tj * stride) + tj;
            w -= pre[qj + 1] - pre[qj + 1 - (reps - 1 - t)];
        }
        o[k] = neg ? 0u - w : w;
    }
}

__global__ __launch_bounds__(64 * kSpreadWavesPerBlock) void trlwe_spread_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ in,
                                                                                 int polys, int stride, int reps)
{
    __shared__ uint32_t coef[kSpreadWavesPerBlock][kN];
    __shared__ uint32_t pre[kSpreadWavesPerBlock][kN + 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int poly = blockIdx.x * kSpreadWavesPerBlock + wave;
    const bool live = poly < polys;
    trlwe_spread_wave(out + (size_t)(live ? poly : 0) * kN, in + (size_t)(live ? poly : 0) * kN, live, stride, reps, coef[wave], pre[wave], lane);
}

// The recorded form (cufhe_amd_enqueue_spread; lut.inc.h: lower_lut_ops): TRLWE g = polynomials 2g and 2g + 1 is read from d[g].in and
// written to d[g].out with its OWN (stride, reps) -- recorded handles live in scattered buffers.  The wave index and the descriptor are
// taken through readfirstlane, so the descriptor is a scalar load and len, big and split of the shared body stay in SGPRs as in the kernel
// above.  d[g].out must not overlap any d[.].in of the launch (the scheduler never puts a writer of a buffer in the level of a reader).
struct SpreadDesc { const uint32_t* in; uint32_t* out; int stride, reps; };
__global__ __launch_bounds__(64 * kSpreadWavesPerBlock) void trlwe_spread_desc_kernel(const SpreadDesc* __restrict__ d, int polys)
{
    __shared__ uint32_t coef[kSpreadWavesPerBlock][kN];
    __shared__ uint32_t pre[kSpreadWavesPerBlock][kN + 1];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int poly = blockIdx.x * kSpreadWavesPerBlock + wave;
    const bool live = poly < polys;
    const SpreadDesc* e = d + ((live ? poly : 0) >> 1);
    const int stride = live ? __builtin_amdgcn_readfirstlane(e->stride) : 1;
    const int reps = live ? __builtin_amdgcn_readfirstlane(e->reps) : 1;
    const size_t half = (size_t)(poly & 1) * kN;
    trlwe_spread_wave(e->out + half, e->in + half, live, stride, reps, coef[wave], pre[wave], lane);
}

}  // namespace cufhe_amd
