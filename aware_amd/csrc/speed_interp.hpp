// Catmull-Rom interpolation at a 16.16 fixed-point position: the weights and the order of the fused multiply-adds that the
// speed change (loop_speed_kernels.hip), the pitch shift (loop_pitch_kernels.hip), the speed search's views
// (speed_search_kernels.hip) and the time warp (loop_warp_kernels.hip) share, so that they give the same bits.  DESIGN.md
// sections 17, 19, 27 and 35.
#pragma once

#include <hip/hip_runtime.h>

namespace aware {

struct SpeedWeights { float wm1, w0, w1, w2; };

// explicit fused multiply-adds, so that every instantiation rounds the same way
__device__ __forceinline__ SpeedWeights speed_weights(float f) {
    SpeedWeights w;
    w.wm1 = (fmaf(2.f - f, f, -1.f) * f) * 0.5f;              // ((-f + 2) f - 1) f / 2
    w.w0 = fmaf(fmaf(3.f, f, -5.f), f * f, 2.f) * 0.5f;       // ((3 f - 5) f^2 + 2) / 2
    w.w1 = (fmaf(fmaf(-3.f, f, 4.f), f, 1.f) * f) * 0.5f;     // ((-3 f + 4) f + 1) f / 2
    w.w2 = ((f - 1.f) * (f * f)) * 0.5f;                      // (f - 1) f^2 / 2
    return w;
}

// the weights at the fraction of the position p
__device__ __forceinline__ SpeedWeights speed_weights_at(long long p) {
    return speed_weights((float)(unsigned)(p & 0xFFFF) * (1.0f / 65536.0f));
}

// a, b, c, d: the samples at i0 - 1, i0, i0 + 1, i0 + 2, zero outside the clip
__device__ __forceinline__ float speed_mix(const SpeedWeights& w, float a, float b, float c, float d) {
    return fmaf(w.w2, d, fmaf(w.w1, c, fmaf(w.w0, b, w.wm1 * a)));
}

// the clip x of n samples read at the position p >= 0 in 16.16 fixed point; zero past the clip's last sample
__device__ __forceinline__ float speed_tap_at(const float* __restrict__ x, int n, long long p) {
    if (p > ((long long)(n - 1) << 16)) return 0.f;
    const int i0 = (int)(p >> 16);                            // 0 <= i0 <= n - 1
    const SpeedWeights w = speed_weights_at(p);
    const float a = i0 >= 1 ? x[i0 - 1] : 0.f;
    const float b = x[i0];
    const float c = i0 + 1 < n ? x[i0 + 1] : 0.f;
    const float d = i0 + 2 < n ? x[i0 + 2] : 0.f;
    return speed_mix(w, a, b, c, d);
}
// output i of a clip x of n samples played at R / 65536 of its speed
__device__ __forceinline__ float speed_tap(const float* __restrict__ x, int n, long long R, int i) {
    return speed_tap_at(x, n, (long long)i * R);
}

// The transposed resampling in gather form: g[0 .. 3] = gu[j0 .. j0 + 3] from gy[0 .. n_out), u being n samples long; the at
// most ten inputs that can reach the four, in ascending order
__device__ __forceinline__ void speed_adjoint4(const float* __restrict__ gy, int n_out, int n, long long R, int j0, float g[4]) {
    g[0] = g[1] = g[2] = g[3] = 0.f;
    const long long lo = ((long long)j0 - 2) << 16, plim = (long long)(n - 1) << 16;
    int i = lo <= 0 ? 0 : (int)(((unsigned long long)lo + (unsigned long long)R - 1ull) / (unsigned long long)R);
    for (; i < n_out; ++i) {
        const long long p = (long long)i * R;
        const int i0 = (int)(p >> 16);
        if (p > plim || i0 > j0 + 4) break;
        const SpeedWeights w = speed_weights_at(p);
        const float v = gy[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int t = j0 + e - i0;
            const float wt = t == -1 ? w.wm1 : (t == 0 ? w.w0 : (t == 1 ? w.w1 : w.w2));
            if (t >= -1 && t <= 2) g[e] = fmaf(wt, v, g[e]);
        }
    }
}

}  // namespace aware
