// Shift search in detection (EXTENSION, parity unpinned: the reference detects a clip as it is): every clip moved by n_views
// candidate frequency shifts in one launch, for the detector to read them all and keep the view it is most confident about
// (aware_sync_select).  DESIGN.md section 39; the restatement is aware_amd/detection/sync.py and, per view,
// aware_amd/embedding/loop_attacks.py::frequency_shift at the start phase 0.
//
//   view (b, j):  out[out_off[b * n_views + j] + i] = x_b[i] cos phi_i - (H x_b)[i] sin phi_i,  i < n_b,
//                 phi_i = 2 pi ((i d[j]) mod 2^20) / 2^20
//
// H x does not depend on d: a workgroup owns one tile of 4096 samples of one clip, computes H x once through the tile body of
// frequency_shift_kernel (shift_hilbert.hpp: the same taps, the same order of accumulation), keeps each thread's 16 values of
// H x and its 16 centre samples in registers, and then writes the tile of every view: per output one sincospif, the
// combination fmaf(-hx, sn, c * cs) of the stand-alone kernel, and a store.  So a view equals aware_frequency_shift at d[j]
// and p0 = 0 bit for bit, and d[j] = 0 gives the clip itself (sincospif(0) is (0, 1)).  A thread's 16 outputs are consecutive:
// four float4 stores where the row is aligned so (rows start at multiples of four floats, out_off, from the host), consecutive
// lanes writing consecutive 64-byte pieces; by element otherwise and at the clip's end: nothing is written between the rows.
// The kernel is bound by its stores, B n_views n floats.  No atomics, no scratch.
#include "common.hpp"
#include "kernels.h"
#include "shift_hilbert.hpp"

namespace aware {

namespace {

__global__ __launch_bounds__(kFsThreads) void shift_views_kernel(const float* __restrict__ in, const int* __restrict__ in_off,
                                                                 const int* __restrict__ in_len, const int* __restrict__ d,
                                                                 int n_views, float* __restrict__ out,
                                                                 const int* __restrict__ out_off) {
    __shared__ float xs[2 * kFsPlanePhys];      // P1 (odd staged samples), then P0
    __shared__ __attribute__((aligned(16))) float hs[kFsTaps];       // g[u] = h[127 - 2 u]
    const int b = blockIdx.y;
    const int t = threadIdx.x;
    const int n = in_len[b];
    const int t0 = blockIdx.x * kFsTile;        // even
    if (t0 >= n) return;
    const int len = min(kFsTile, n - t0);
    const float* __restrict__ x = in + (size_t)in_off[b];
    float* p1 = xs;
    float* p0s = xs + kFsPlanePhys;
    fs_taps(hs, t);
    fs_stage<false>(x, n, t0, len, 0, 0, p1, p0s, t);
    const int o = kFsPer * t;
    if (o >= ((len + 1) >> 1)) return;          // the whole wave, but for the last one of a ragged tile; no barrier follows
    v2f acc[kFsPer];
    fs_hilbert(p1, p0s, hs, t, acc);
    const int j0 = 2 * o;                       // the first of this thread's 16 outputs, from t0
    float hx[2 * kFsPer], c[2 * kFsPer];
#pragma unroll
    for (int m = 0; m < kFsPer; ++m) {
        hx[2 * m] = acc[m].x; hx[2 * m + 1] = acc[m].y;
    }
#pragma unroll
    for (int v = 0; v < 2 * kFsPer; ++v) c[v] = j0 + v < len ? x[t0 + j0 + v] : 0.f;
    const bool whole = j0 + 2 * kFsPer <= len;
    for (int j = 0; j < n_views; ++j) {
        const int dj = d[j];
        if (dj < -kShiftMax || dj > kShiftMax) continue;              // a shift outside the operator's range: no view
        float* yo = out + (size_t)out_off[(size_t)b * n_views + j] + t0 + j0;
        float r[2 * kFsPer];
#pragma unroll
        for (int v = 0; v < 2 * kFsPer; ++v) {
            r[v] = 0.f;
            if (j0 + v < len) {
                float sn, cs;
                sincospif(fs_phase(0, dj, t0 + j0 + v), &sn, &cs);
                r[v] = fmaf(-hx[v], sn, c[v] * cs);
            }
        }
        if (whole && (((size_t)yo) & 15) == 0) {
#pragma unroll
            for (int v = 0; v < kFsPer / 2; ++v) ((float4*)yo)[v] = make_float4(r[4 * v], r[4 * v + 1], r[4 * v + 2], r[4 * v + 3]);
        } else {
#pragma unroll
            for (int v = 0; v < 2 * kFsPer; ++v)
                if (j0 + v < len) yo[v] = r[v];
        }
    }
}

}  // namespace

void launch_shift_views(const float* in, const int* in_off, const int* in_len, int B, const int* d, int n_views, float* out,
                        const int* out_off, int max_len, hipStream_t st) {
    const unsigned gx = (unsigned)(((long long)max_len + kFsTile - 1) / kFsTile);
    hipLaunchKernelGGL(shift_views_kernel, dim3(gx, (unsigned)B), dim3(kFsThreads), 0, st, in, in_off, in_len, d, n_views, out,
                       out_off);
}

}  // namespace aware
