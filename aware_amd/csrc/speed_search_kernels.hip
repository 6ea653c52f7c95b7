// Speed search in detection (EXTENSION, parity unpinned: the reference detects a clip as it is): every clip resampled at
// n_views candidate speeds in one launch, for the detector to read them all and keep the view it is most confident about
// (aware_sync_select).  DESIGN.md section 27; the restatement is aware_amd/detection/sync.py and, per view,
// aware_amd/embedding/loop_attacks.py::speed_change with n_out = speed_length.
//
//   view (b, j):  R = 65536 + m[j],  n_out = ((n_b - 1) << 16) / R + 1  (64-bit; every position i R then lies inside the clip),
//   out[out_off[b * n_views + j] + i] = the Catmull-Rom tap of speed_interp.hpp at p_i = i R,  i < n_out
//
// so a view equals aware_speed_change at the same m and length bit for bit, and m = 0 copies the clip.  A workgroup owns
// 1024 consecutive outputs of one view, a thread four.  The inputs those read are one span of at most
// 1023 R / 65536 + 5 samples, staged in LDS by coalesced loads (zero outside the clip); the taps come from LDS.  Rows start
// at multiples of four floats (out_off, from the host), so whole groups are stored as float4 (by element where a row is not
// aligned so); the last partial group is stored by element: nothing is written between the rows.  No atomics, no scratch.
#include "common.hpp"
#include "kernels.h"
#include "speed_interp.hpp"

namespace aware {

namespace {

constexpr int kSvThreads = 256;
constexpr int kSvTile = 4 * kSvThreads;
// floats of LDS: the span of a tile at the largest ratio, (1023 * (65536 + kSpeedMax) >> 16) + 5 = 1293, rounded up
constexpr int kSvSpan = (int)(((long long)(kSvTile - 1) * (65536 + kSpeedMax)) >> 16) + 8;
static_assert(kSvSpan * sizeof(float) < 8192, "the staged span stays under 8 KB of LDS");

__global__ __launch_bounds__(kSvThreads) void speed_views_kernel(const float* __restrict__ in, const int* __restrict__ in_off,
                                                                 const int* __restrict__ in_len, const int* __restrict__ m,
                                                                 int n_views, float* __restrict__ out,
                                                                 const int* __restrict__ out_off) {
    __shared__ float span[kSvSpan];
    const int j = blockIdx.y, b = blockIdx.z;
    const int n = in_len[b], mj = m[j];
    if (n < 1 || mj < kSpeedMin || mj > kSpeedMax) return;            // an offset outside the operator's range: no view
    const long long R = 65536 + (long long)mj;
    const int n_out = (int)((((long long)n - 1) << 16) / R) + 1;      // <= 1.27 n
    const int t0 = blockIdx.x * kSvTile;
    if (t0 >= n_out) return;
    const float* x = in + (size_t)in_off[b];
    float* y = out + (size_t)out_off[(size_t)b * n_views + j];
    const int i = t0 + 4 * threadIdx.x;
    float v[4];
    if (mj == 0) {
        // the identity, exactly
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = i + e < n_out ? x[i + e] : 0.f;
    } else {
        const int t1 = min(t0 + kSvTile, n_out) - 1;                  // the tile's last output
        const int s0 = (int)(((long long)t0 * R) >> 16) - 1;          // the first and the last sample a tap of the tile reads
        const int cnt = (int)(((long long)t1 * R) >> 16) + 2 - s0 + 1;            // <= kSvSpan - 3
        for (int k = threadIdx.x; k < cnt; k += kSvThreads) {
            const int g = s0 + k;
            span[k] = g >= 0 && g < n ? x[g] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = 0.f;
            if (i + e < n_out) {
                const long long p = (long long)(i + e) * R;           // <= (n - 1) << 16: inside the clip
                const float* s = span + ((int)(p >> 16) - 1 - s0);
                v[e] = speed_mix(speed_weights_at(p), s[0], s[1], s[2], s[3]);
            }
        }
    }
    if (i + 3 < n_out && (reinterpret_cast<size_t>(y + i) & 15) == 0) {
        *reinterpret_cast<float4*>(y + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i + e < n_out) y[i + e] = v[e];
    }
}

}  // namespace

void launch_speed_views(const float* in, const int* in_off, const int* in_len, int B, const int* m, int n_views, float* out,
                        const int* out_off, int max_len, hipStream_t st) {
    const unsigned gx = (unsigned)(((long long)max_len + kSvTile - 1) / kSvTile);
    hipLaunchKernelGGL(speed_views_kernel, dim3(gx, (unsigned)n_views, (unsigned)B), dim3(kSvThreads), 0, st, in, in_off,
                       in_len, m, n_views, out, out_off);
}

}  // namespace aware
