// Overlap-add of Hann-windowed segments taken at the rate Q / 65536, four consecutive samples at a time: the arithmetic and
// the order of the fused multiply-adds that the time stretch (loop_stretch_kernels.hip) and the pitch shift
// (loop_pitch_kernels.hip) share, so that the two give the same bits.  DESIGN.md sections 18 and 19.
//
//   H = 256, N = 1024, w the periodic Hann window of N points in f32,  a_t = (t H Q) >> 16 (64-bit, arithmetic) for t >= -2
//   forward   u[k] = 1/2 sum over ascending t of w[k - t H + 512] x[k - t H + a_t],   0 <= k - t H + 512 < N (four t)
//   adjoint   gx[j] = 1/2 sum over ascending t of w[j - a_t + 512] gu[j - a_t + t H],  0 <= j - a_t + 512 < N (at most six t)
#pragma once
#include "common.hpp"

namespace aware {

constexpr int kOlaHop = 256, kOlaWin = 1024;
static_assert(kOlaHop == kHop && kOlaHop % 4 == 0, "four consecutive samples share their frames");
// a_t = (t H Q) >> 16: where segment t of the input starts (its centre, with the window's 512 taken off both sides)
__device__ __forceinline__ long long ola_pos(long long t, long long Q) { return (t * kOlaHop * Q) >> 16; }

// the first frame t >= -2 with a_t >= j - 511: the ceiling of (j - 511) 256 / Q (a division of a negative numerator truncates
// towards zero, which is its ceiling)
__device__ __forceinline__ long long ola_first_frame(int j, long long Q) {
    const long long num = ((long long)j - (kOlaWin / 2 - 1)) * kOlaHop;
    const long long t = num > 0 ? (num + Q - 1) / Q : num / Q;
    return t < -2 ? -2 : t;
}

// u[k0 .. k0 + 3] from x[0 .. n), k0 a multiple of four: the four windowed reads in ascending t, then the halving.  CAP: u ends
// at Lu, zero outside [0, Lu); without it u has no end, k0 >= 0, Lu is not read and the kernel holds no code of the cap
template <bool CAP>
__device__ __forceinline__ void ola_forward4(const float* __restrict__ x, int n, const float* __restrict__ w, long long Q,
                                             int Lu, int k0, float v[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (CAP && (k0 < 0 || k0 >= Lu)) return;
    const int tmax = (k0 + kOlaWin / 2) / kOlaHop;            // the last frame whose window holds k0 .. k0 + 3
#pragma unroll
    for (int k = 3; k >= 0; --k) {
        const int t = tmax - k;                               // >= -1
        const int wi = k0 - t * kOlaHop + kOlaWin / 2;        // 0 <= wi, wi + 3 < 1024
        const long long src = (long long)(k0 - t * kOlaHop) + ola_pos(t, Q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long long s = src + e;
            if (s >= 0 && s < n) v[e] = fmaf(w[wi + e], x[s], v[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] *= 0.5f;
    if (CAP) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k0 + e >= Lu) v[e] = 0.f;
    }
}

// gx[j0 .. j0 + 3] from gu[shift .. shift + count) at src, zero outside: the at most seven frames whose segment reaches one
// of the four, in ascending t
__device__ __forceinline__ void ola_adjoint4(const float* __restrict__ src, int count, int shift, const float* __restrict__ w,
                                             long long Q, int j0, float g[4]) {
    g[0] = g[1] = g[2] = g[3] = 0.f;
    for (long long t = ola_first_frame(j0, Q);; ++t) {
        const long long at = ola_pos(t, Q);
        if (at > (long long)j0 + 3 + kOlaWin / 2) break;
        const long long wi = (long long)j0 - at + kOlaWin / 2;              // window index of output j0
        const long long o = (long long)j0 - at + t * kOlaHop - shift;       // the sample of gu that reaches it, in src
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (wi + e >= 0 && wi + e < kOlaWin && o + e >= 0 && o + e < count) g[e] = fmaf(w[wi + e], src[o + e], g[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] *= 0.5f;
}

}  // namespace aware
