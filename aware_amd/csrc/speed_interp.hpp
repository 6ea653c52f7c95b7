// Catmull-Rom interpolation at a 16.16 fixed-point position: the weights and the order of the fused multiply-adds that the
// speed change (loop_speed_kernels.hip) and the speed search's views (speed_search_kernels.hip) share, so that the two give
// the same bits.  DESIGN.md sections 17 and 27.
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

// output i of a clip x of n samples played at R / 65536 of its speed; zero past the clip's last sample
__device__ __forceinline__ float speed_tap(const float* __restrict__ x, int n, long long R, int i) {
    const long long p = (long long)i * R;
    if (p > ((long long)(n - 1) << 16)) return 0.f;
    const int i0 = (int)(p >> 16);                            // 0 <= i0 <= n - 1
    const SpeedWeights w = speed_weights_at(p);
    const float a = i0 >= 1 ? x[i0 - 1] : 0.f;
    const float b = x[i0];
    const float c = i0 + 1 < n ? x[i0 + 1] : 0.f;
    const float d = i0 + 2 < n ? x[i0 + 2] : 0.f;
    return speed_mix(w, a, b, c, d);
}

}  // namespace aware
