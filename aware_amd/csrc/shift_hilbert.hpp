// The tile body of the frequency shift's 255-tap Hilbert transformer, shared by frequency_shift_kernel (loop_shift_kernels.hip,
// where the layout is derived) and shift_views_kernel (shift_search_kernels.hip): the constants of a tile, the staging of a
// tile into the two de-interleaved LDS planes, the 64 tap magnitudes and the 128 packed FMAs per pair of outputs.  One
// statement, so that both kernels round every Hx alike: a view of the shift search equals aware_frequency_shift bit for bit.
#pragma once
#include "common.hpp"
#include "loop_limits.hpp"

namespace aware {

constexpr int kFsThreads = 256;
constexpr int kFsPer = 8;                       // outputs per thread and parity
constexpr int kFsTile = 2 * kFsPer * kFsThreads;        // 4096 outputs per workgroup and pass
constexpr int kFsTaps = kFilterHalf + 1;                // 128 steps of the window: the odd taps
constexpr int kFsPlane = kFsTile / 2 + kFsTaps + 2 * kFsPer;    // staged samples per plane: tile, halo, the last window's overshoot
constexpr int kFsPlanePhys = 2480;              // >= kFsPlane + (kFsPlane >> 3) + 1, and 16 mod 32
static_assert(kFsPlanePhys >= kFsPlane + (kFsPlane >> 3) + 1 && kFsPlanePhys % 32 == 16, "the planes' padding and bank offset");

typedef float v2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int fs_phys(int p) { return p + (p >> 3); }

// phi_i in half turns: theta_i 2^-19, exact in f32
__device__ __forceinline__ float fs_phase(int p0, int d, int i) {
    const unsigned theta = ((unsigned)p0 + (unsigned)i * (unsigned)d) & 0xFFFFFu;
    return (float)theta * (1.f / 524288.f);
}

// hs[u] = g[u] = h[127 - 2 u], u < 128, by the threads t < 64; a barrier must follow before hs is read
__device__ __forceinline__ void fs_taps(float* hs, int t) {
    if (t < kFsTaps / 2) {                      // the 64 distinct magnitudes: k = 127 - 2 t, odd, 127 down to 1
        const int k = kFilterHalf - 2 * t;
        const float w = 0.54f + 0.46f * cospif((float)k * (1.f / 127.f));
        const float h = w * 2.f / (3.14159265358979323846f * (float)k);
        hs[t] = h; hs[kFsTaps - 1 - t] = -h;    // g[127 - u] = h[2 u - 127] = -g[u]
    }
}

// The tile of `len` outputs from the even sample t0 of the clip x of n samples, into the planes p1 (odd staged samples) and
// p0s: staged sample q is x[t0 - 128 + q], of the parity of q, zero outside the clip; with SINE it is multiplied by
// sin phi_i (the adjoint).  A barrier on either side: the pass before is done with the planes, and the planes are whole.
template <bool SINE>
__device__ __forceinline__ void fs_stage(const float* __restrict__ x, int n, int t0, int len, int p0, int d, float* p1,
                                         float* p0s, int t) {
    __syncthreads();
    for (int q = t; q < len + 2 * kFsTaps + 4 * kFsPer; q += kFsThreads) {
        const int i = t0 - kFsTaps + q;
        float v = 0.f;
        if (i >= 0 && i < n) {
            v = x[i];
            if (SINE) v *= sinpif(fs_phase(p0, d, i));
        }
        ((q & 1) ? p1 : p0s)[fs_phys(q >> 1)] = v;
    }
    __syncthreads();
}

// Thread t's 8 pairs of outputs, pair a = 8 t + m: acc[m].x = Hx[2 a] from P1[a + u], acc[m].y = Hx[2 a + 1] from
// P0[a + 1 + u], u = 0..127 in ascending order, one packed FMA per tap on both.  The two windows slide through registers.
__device__ __forceinline__ void fs_hilbert(const float* p1, const float* p0s, const float* hs, int t, v2f (&acc)[kFsPer]) {
    const float* lo = p1 + 9 * t;               // fs_phys(8 t + c) = 9 t + fs_phys(c)
    const float* hi = p0s + 9 * t;
    v2f w[kFsPer];
#pragma unroll
    for (int m = 0; m < kFsPer; ++m) { acc[m] = (v2f){0.f, 0.f}; w[m] = (v2f){lo[fs_phys(m)], hi[fs_phys(m + 1)]}; }
    for (int u = 0; u < kFsTaps / kFsPer; ++u) {
        const float4 ha = ((const float4*)hs)[2 * u], hb = ((const float4*)hs)[2 * u + 1];
        const float h8[kFsPer] = {ha.x, ha.y, ha.z, ha.w, hb.x, hb.y, hb.z, hb.w};
#pragma unroll
        for (int s = 0; s < kFsPer; ++s) {
            const float h = h8[s];              // g[8 u + s]
#pragma unroll
            for (int m = 0; m < kFsPer; ++m) acc[m] += h * w[m];
#pragma unroll
            for (int m = 0; m < kFsPer - 1; ++m) w[m] = w[m + 1];
            w[kFsPer - 1] = (v2f){lo[9 * (u + 1) + s], hi[9 * (u + 1) + fs_phys(s + 1)]};
        }
    }
}

}  // namespace aware
