// Band filter (EXTENSION, parity unpinned: the reference has LowPassFilter, HighPassFilter and RandomBandstop as post-hoc IIR
// attacks only and no chain inside its loop): a zero-phase windowed-sinc FIR of 255 taps with edges and response drawn per clip.
// DESIGN.md section 25; the torch restatement is aware_amd/embedding/loop_attacks.py::filter_taps / band_filter / apply_chain.
//
//   r = philox4x32_10((0, s, 1 + j, 1), (seed_b, 0x5EED)),  on = (r0 + 0.5) / 2^32 < prob,
//   e1 = c_lo + ((r1 * (c_hi - c_lo + 1)) >> 32), e2 the same from r2, in units of 1 / 65536 cycle per sample
//   response = the ((r3 * popcount(mask)) >> 32)-th set bit of mask (1 lowpass, 2 highpass, 4 bandpass, 8 bandstop)
//   lowpass, highpass: c1 = e1;  band responses: c1 = min(e1, e2), c2 = max(max(e1, e2), c1 + w_min)
//   w[k] = 0.54 + 0.46 cos(pi k / 127),  lp_c[0] = c / 32768,  lp_c[k] = w[k] sin(2 pi ((c |k|) mod 65536) / 65536) / (pi |k|)
//   h = lp_c1 | delta - lp_c1 | lp_c2 - lp_c1 | delta - (lp_c2 - lp_c1)
//   z[i] = sum_{k = -127..127} h[k] x[i - k], x zero outside the clip
//
// h is symmetric and the extension is by zeros, so the operator is its own adjoint: the backward pass is this kernel on the
// gradient with the same draw.  One kernel for both layouts.  A workgroup serves up to kFbTile consecutive outputs at a time:
// it stages them with 127 samples of halo on each side into LDS (zeros outside the clip, whatever lies beside it in memory),
// builds the 128 distinct taps, and every thread produces 8 consecutive outputs in the lower half of the tile and the 8 at the
// same place in the upper half.  The two share their taps, so each tap is one packed FMA on both: 16 FMAs per three LDS reads
// (one sample of each half and the broadcast tap).  The window of 8 samples slides through registers.  LDS index q lives at
// q + (q >> 3): thread t reads 8 t + const, which would put a wave on 8 banks; with the padding its stride is 9.
#include "loop_stage.hpp"

namespace aware {

namespace {

constexpr int kFbThreads = 256;
constexpr int kFbPer = 8;                       // consecutive outputs per thread and half
constexpr int kFbTile = 2 * kFbPer * kFbThreads;        // 4096 outputs per workgroup and pass
constexpr int kFbLogical = kFbTile + 2 * kFilterHalf + 2 * kFbPer;      // staged samples: tile, halo, and the last window's overshoot
constexpr int kFbLds = kFbLogical + (kFbLogical >> 3) + 8;

typedef float v2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int fb_phys(int q) { return q + (q >> 3); }

// the windowed-sinc low-pass at the edge c, tap k >= 0
__device__ __forceinline__ float fb_lowpass(int c, int k) {
    if (k == 0) return (float)c * (1.f / 32768.f);
    const int p = (c * k) & 65535;              // the phase in 1 / 65536 turn: c < 2^15 and k < 2^7, no overflow
    const float w = 0.54f + 0.46f * cospif((float)k * (1.f / 127.f));
    return w * sinpif((float)p * (1.f / 32768.f)) / (3.14159265358979323846f * (float)k);
}
// tap |k| of the response (one bit) at the edges c1, c2
__device__ __forceinline__ float fb_tap(int response, int c1, int c2, int k) {
    const float d = k == 0 ? 1.f : 0.f;
    const float l1 = fb_lowpass(c1, k);
    if (response == 1) return l1;
    if (response == 2) return d - l1;
    const float band = fb_lowpass(c2, k) - l1;
    return response == 4 ? band : d - band;
}

template <bool LOOP>
__global__ __launch_bounds__(kFbThreads) void band_filter_kernel(FilterLaunch a) {
    __shared__ float xs[kFbLds];
    __shared__ __attribute__((aligned(16))) float hs[2 * kFilterHalf + 2];      // tap k at k + 127, and a zero for the 256th step of the window
    const int b = blockIdx.y;
    const int t = threadIdx.x;
    const float* __restrict__ x;
    float* __restrict__ y;
    int n, i0, i1, response, c1, c2;            // the clip's length, this workgroup's outputs [i0, i1), the filter (response 0: a copy)
    if (LOOP) {
        LoopStage s;
        if (!loop_stage_enter(a.draw, b, s)) return;
        x = a.in + s.so; y = a.out + s.so;
        n = s.n;
        i0 = s.jb0 * kHop; i1 = s.jb1 * kHop;
        const int e1 = loop_uniform(s.r[1], a.c_lo, a.c_hi), e2 = loop_uniform(s.r[2], a.c_lo, a.c_hi);
        int pick = loop_below(s.r[3], __popc((unsigned)a.mask));
        response = 0;
        for (int bit = 1; bit <= 8; bit <<= 1)
            if (a.mask & bit) { if (pick == 0) response = bit; --pick; }
        if (!s.on) response = 0;
        if (response >= 4) { c1 = min(e1, e2); c2 = max(max(e1, e2), c1 + a.w_min); }
        else { c1 = e1; c2 = e1; }
    } else {
        n = a.len[b];
        i0 = blockIdx.x * kFbTile;
        if (i0 >= n) return;
        i1 = min(i0 + kFbTile, n);
        x = a.in + a.off[b]; y = a.out + a.off[b];
        const int rs = a.response[b] & 15;
        response = rs & -rs;                    // its lowest bit; none: a copy
        c1 = min(max(a.c1[b], 0), 32767); c2 = min(max(a.c2[b], 0), 32767);
    }
    if (response == 0) {
        for (int i = i0 + t; i < i1; i += kFbThreads) y[i] = x[i];
        return;
    }
    if (t <= kFilterHalf) {                     // the 128 distinct taps, mirrored
        const float h = fb_tap(response, c1, c2, t);
        hs[kFilterHalf - t] = h; hs[kFilterHalf + t] = h;
        if (t == 0) hs[2 * kFilterHalf + 1] = 0.f;
    }
    if (!LOOP && a.taps && blockIdx.x == 0) {
        const int k = t - kFilterHalf;
        a.taps[(size_t)b * 256 + t] = t < 2 * kFilterHalf + 1 ? fb_tap(response, c1, c2, k < 0 ? -k : k) : 0.f;
    }
    for (int t0 = i0; t0 < i1; t0 += kFbTile) {
        const int len = min(kFbTile, i1 - t0);
        const int half = ((len + 2 * kFbPer - 1) / (2 * kFbPer)) * kFbPer;      // a multiple of 8, half <= 2048, len - half <= half
        __syncthreads();                        // the pass before is done with xs
        // staged sample q is x[t0 - 127 + q]: zero outside the clip
        for (int q = t; q < len + 2 * kFilterHalf + 2 * kFbPer; q += kFbThreads) {
            const int i = t0 - kFilterHalf + q;
            xs[fb_phys(q)] = (i >= 0 && i < n) ? x[i] : 0.f;
        }
        __syncthreads();
        const int o = kFbPer * t;
        if (o >= half) continue;                // the whole wave, but for the last one of a ragged tile
        // out[m] = sum_jj h[|127 - jj|] X[o + m + jj], jj = 0..254; the lower half in .x, the upper in .y
        const float* lo = xs + 9 * t;           // fb_phys(o + c) = 9 t + fb_phys(c)
        const float* hi = lo + fb_phys(half);
        v2f acc[kFbPer], w[kFbPer];
#pragma unroll
        for (int m = 0; m < kFbPer; ++m) { acc[m] = (v2f){0.f, 0.f}; w[m] = (v2f){lo[m], hi[m]}; }
        for (int u = 0; u < 32; ++u) {
            const float4 ha = ((const float4*)hs)[2 * u], hb = ((const float4*)hs)[2 * u + 1];
            const float h8[kFbPer] = {ha.x, ha.y, ha.z, ha.w, hb.x, hb.y, hb.z, hb.w};
#pragma unroll
            for (int s = 0; s < kFbPer; ++s) {
                const float h = h8[s];          // tap 127 - jj of step jj = 8 u + s: the table is symmetric
#pragma unroll
                for (int m = 0; m < kFbPer; ++m) acc[m] += h * w[m];
#pragma unroll
                for (int m = 0; m < kFbPer - 1; ++m) w[m] = w[m + 1];
                w[kFbPer - 1] = (v2f){lo[9 * (u + 1) + s], hi[9 * (u + 1) + s]};
            }
        }
        float* ylo = y + t0 + o;
        float* yhi = ylo + half;
        const int nlo = min(kFbPer, min(half, len) - o), nhi = min(kFbPer, len - half - o);      // half > len in a tile of under 8 samples
        if (nlo == kFbPer && (((size_t)ylo) & 15) == 0) {
            ((float4*)ylo)[0] = make_float4(acc[0].x, acc[1].x, acc[2].x, acc[3].x);
            ((float4*)ylo)[1] = make_float4(acc[4].x, acc[5].x, acc[6].x, acc[7].x);
        } else {
#pragma unroll
            for (int m = 0; m < kFbPer; ++m)
                if (m < nlo) ylo[m] = acc[m].x;
        }
        if (nhi == kFbPer && (((size_t)yhi) & 15) == 0) {
            ((float4*)yhi)[0] = make_float4(acc[0].y, acc[1].y, acc[2].y, acc[3].y);
            ((float4*)yhi)[1] = make_float4(acc[4].y, acc[5].y, acc[6].y, acc[7].y);
        } else {
#pragma unroll
            for (int m = 0; m < kFbPer; ++m)
                if (m < nhi) yhi[m] = acc[m].y;
        }
    }
}

}  // namespace

void launch_band_filter(const FilterLaunch& L, hipStream_t st) {
    hipLaunchKernelGGL(L.draw.frame_off ? band_filter_kernel<true> : band_filter_kernel<false>, stage_grid(L.draw, L.B, L.max_len, kFbTile),
                       dim3(kFbThreads), 0, st, L);
}

}  // namespace aware
