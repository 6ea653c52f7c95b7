// Short-time objective intelligibility (Taal et al., IEEE TASLP 2011) of a ragged batch of clip pairs at 10 kHz: the
// function aware_amd/metrics/audio.py::stoi computes on the host for one clip, here for every clip of a batch without
// leaving the device (reference: metrics/audio.py:42-64 hands the same two signals to pystoi).
//
//   stoi_energy_kernel    frame energies of the clean signal, 20 log10(|w x_i| + eps)         one wave per frame
//   stoi_scan_kernel      per clip: maximum, keep flags (40 dB range), exclusive scan -> kept-frame list, K_b
//   stoi_bands_kernel     silent-frame removal + re-framing + window + 512-point rFFT + third-octave band sums of
//                         both signals, fused: frame m of the overlap-added signal only depends on kept frames
//                         m - 1, m, m + 1, so the intermediate signal never exists                 one wave per frame
//   stoi_segments_kernel  the 30-frame segment statistics in float64, partial sums per 64 segments
//   stoi_finish_kernel    partials merged in ascending order, divided by segments x 15
//
// Frames, FFT and band sums are float32; energies are compared and segments are computed in float64.  Every reduction
// has a fixed order and touches one clip only: a clip's score does not depend on its neighbours or on the run.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "common.hpp"
#include "fft_any.hpp"
#include "kernels.h"

namespace aware {
namespace {

constexpr int kStoiWaves = 4;
constexpr double kStoiEps = 2.220446049250313e-16;       // np.finfo(np.float64).eps
constexpr double kStoiDyn = 40.0;
constexpr double kStoiClip = 6.623413251903491;          // 1 + 10^(15/20): clipping at -15 dB SDR

// first row of clip b in the per-frame arrays: sum of stoi_frames(n_c), c < b.  All threads of the block call this.
__device__ __forceinline__ int stoi_frame_base(const int* __restrict__ n, int b, int* red) {
    int s = 0;
    for (int c = threadIdx.x; c < b; c += blockDim.x) s += stoi_frames(n[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    s = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return s;
}

// ---- 1. frame energies ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stoi_energy_kernel(StoiLaunch L) {
    __shared__ int red[kStoiWaves];
    const int b = blockIdx.y;
    const int F = stoi_frames(L.n[b]);
    if ((int)blockIdx.x * kStoiWaves >= F) return;
    const int base = stoi_frame_base(L.n, b, red);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float* __restrict__ x = L.clean + L.clean_off[b];
    const float* __restrict__ w = L.tab.window;
    const float w0 = w[4 * lane], w1 = w[4 * lane + 1], w2 = w[4 * lane + 2], w3 = w[4 * lane + 3];
    for (int f = blockIdx.x * kStoiWaves + wv; f < F; f += gridDim.x * kStoiWaves) {
        const float* p = x + (size_t)f * kStoiHop + 4 * lane;            // f*128 + 255 < n: inside the clip
        const float a0 = w0 * p[0], a1 = w1 * p[1], a2 = w2 * p[2], a3 = w3 * p[3];
        float ss = a0 * a0;
        ss += a1 * a1;
        ss += a2 * a2;
        ss += a3 * a3;
        ss = wave_sum(ss);
        if (lane == 0) L.energy[base + f] = 20.0 * log10((double)sqrtf(ss) + kStoiEps);
    }
}

// ---- 2. keep flags and their exclusive scan, one workgroup per clip --------------------------------------------------
__global__ __launch_bounds__(256) void stoi_scan_kernel(StoiLaunch L) {
    __shared__ int red[kStoiWaves];
    __shared__ double dred[kStoiWaves];
    const int b = blockIdx.x;
    const int F = stoi_frames(L.n[b]);
    const int base = stoi_frame_base(L.n, b, red);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double* __restrict__ e = L.energy + base;
    double mx = -INFINITY;
    for (int i = threadIdx.x; i < F; i += 256) mx = fmax(mx, e[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    if (lane == 0) dred[wv] = mx;
    __syncthreads();
    mx = fmax(fmax(dred[0], dred[1]), fmax(dred[2], dred[3]));
    int running = 0;                                      // kept frames before this chunk of 256
    for (int i0 = 0; i0 < F; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const bool keep = i < F && (mx - kStoiDyn - e[i]) < 0.0;
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        __syncthreads();                                  // the previous chunk's reads of red[]
        if (lane == 0) red[wv] = __popcll(m);
        __syncthreads();
        int off = running;
        for (int q = 0; q < wv; ++q) off += red[q];
        if (keep) L.kept[base + off + before] = i;
        running += red[0] + red[1] + red[2] + red[3];
    }
    if (threadIdx.x == 0) {
        L.kcount[b] = running;
        L.fbase[b] = base;
        if (L.kept_out) L.kept_out[b] = running;
    }
}

// ---- 3. re-framed frame m of both signals -> window -> rFFT -> band magnitudes ----------------------------------------
// xs[128 m + o] = xf[m][o] + xf[m - 1][o + 128] (o < 128, m >= 1) or + xf[m + 1][o - 128] (o >= 128), xf[j] = w * (frame
// kept[j] of the signal); m < K - 1, so kept frame m + 1 always exists.
__device__ __forceinline__ void stoi_band_row(const StoiTables& T, const float* __restrict__ x, int f0, int f1, int f2,
                                              bool has_prev, int lane, cf* s, float* pw, const float* w, const cf* th,
                                              float* __restrict__ row) {
    {
        const int o = 2 * lane;                           // first half: the tail of the previous kept frame overlaps
        float v0 = w[o] * x[f1 * kStoiHop + o], v1 = w[o + 1] * x[f1 * kStoiHop + o + 1];
        if (has_prev) {
            v0 += w[o + 128] * x[f0 * kStoiHop + o + 128];
            v1 += w[o + 129] * x[f0 * kStoiHop + o + 129];
        }
        s[lane] = mk(v0 * w[o], v1 * w[o + 1]);
    }
    {
        const int o = 2 * lane + 128;                     // second half: the head of the next kept frame
        const float v0 = w[o] * x[f1 * kStoiHop + o] + w[o - 128] * x[f2 * kStoiHop + o - 128];
        const float v1 = w[o + 1] * x[f1 * kStoiHop + o + 1] + w[o - 127] * x[f2 * kStoiHop + o - 127];
        s[lane + 64] = mk(v0 * w[o], v1 * w[o + 1]);
    }
    s[lane + 128] = mk(0.f, 0.f);                         // the frame is zero-padded at its end to 512 samples
    s[lane + 192] = mk(0.f, 0.f);
    wave_sync();
    fa::fft_wave<256, -1>(lane, s, th);
#pragma unroll
    for (int i = 0; i < 4; ++i) {                         // bins 0..255 (no band reaches bin 256)
        const int k = lane + 64 * i;
        const cf X = fa::rfft_bin<256>(k, s, T.twN);
        pw[k] = X.x * X.x + X.y * X.y;
    }
    wave_sync();
    // four lanes per band: each sums a quarter of the band's run of bins in ascending order, then the four partial sums
    // are merged in a fixed order
    const int band = lane >> 2, part = lane & 3;
    const int lo = T.bands[band], hi = T.bands[kStoiRow + band];
    const int q = (hi - lo + 3) >> 2;
    const int k0 = lo + part * q, k1 = min(hi, k0 + q);
    float acc = 0.f;
    for (int k = k0; k < k1; ++k) acc += pw[k];
    acc += __shfl_xor(acc, 1);
    acc += __shfl_xor(acc, 2);
    if (part == 0) row[band] = sqrtf(acc);                // band 15 (the pad) is empty: 0
    wave_sync();
}

__global__ __launch_bounds__(256) void stoi_bands_kernel(StoiLaunch L) {
    __shared__ cf sbuf[kStoiWaves][256];
    __shared__ float pwbuf[kStoiWaves][256];
    __shared__ cf th[128];
    __shared__ float w[kStoiFrame];
    const int b = blockIdx.y;
    const int K = L.kcount[b];
    if ((int)blockIdx.x * kStoiWaves >= K - 1) return;
    for (int i = threadIdx.x; i < 128; i += blockDim.x) th[i] = L.tab.th[i];
    w[threadIdx.x] = L.tab.window[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int m = blockIdx.x * kStoiWaves + wv;
    if (m >= K - 1) return;
    const int base = L.fbase[b];
    const int* __restrict__ kept = L.kept + base;
    const int f1 = kept[m], f2 = kept[m + 1], f0 = m > 0 ? kept[m - 1] : 0;
    const size_t r = (size_t)(base + m) * kStoiRow;
    stoi_band_row(L.tab, L.clean + L.clean_off[b], f0, f1, f2, m > 0, lane, sbuf[wv], pwbuf[wv], w, th, L.xt + r);
    stoi_band_row(L.tab, L.proc + L.proc_off[b], f0, f1, f2, m > 0, lane, sbuf[wv], pwbuf[wv], w, th, L.yt + r);
}

// ---- 4. segments: thread = (segment, band), 16 x 16 per pass, 64 segments per workgroup ------------------------------
__global__ __launch_bounds__(256) void stoi_segments_kernel(StoiLaunch L) {
    __shared__ double red[kStoiWaves];
    const int b = blockIdx.y;
    const int nseg = L.kcount[b] - 1 - (kStoiN - 1);       // re-framed frames K - 1, segments end at m = 30 .. K - 1
    if ((int)blockIdx.x * kStoiSegChunk >= nseg) return;
    const int base = L.fbase[b];
    const int band = threadIdx.x & 15, sl = threadIdx.x >> 4;
    double acc = 0.0;
    for (int it = 0; it < kStoiSegChunk / 16; ++it) {
        const int seg = blockIdx.x * kStoiSegChunk + it * 16 + sl;
        if (seg >= nseg || band >= kStoiBands) continue;
        const float* __restrict__ xr = L.xt + (size_t)(base + seg) * kStoiRow + band;
        const float* __restrict__ yr = L.yt + (size_t)(base + seg) * kStoiRow + band;
        float xv[kStoiN], yv[kStoiN];
#pragma unroll
        for (int i = 0; i < kStoiN; ++i) { xv[i] = xr[i * kStoiRow]; yv[i] = yr[i * kStoiRow]; }
        double sx2 = 0.0, sy2 = 0.0, sx = 0.0;
#pragma unroll
        for (int i = 0; i < kStoiN; ++i) {
            const double x = xv[i], y = yv[i];
            sx2 += x * x; sy2 += y * y; sx += x;
        }
        const double a = sqrt(sx2) / (sqrt(sy2) + kStoiEps);
        double syp = 0.0;
#pragma unroll
        for (int i = 0; i < kStoiN; ++i) syp += fmin((double)yv[i] * a, (double)xv[i] * kStoiClip);
        const double mx = sx / kStoiN, my = syp / kStoiN;
        double cxx = 0.0, cyy = 0.0, cxy = 0.0;
#pragma unroll
        for (int i = 0; i < kStoiN; ++i) {
            const double xc = (double)xv[i] - mx;
            const double yc = fmin((double)yv[i] * a, (double)xv[i] * kStoiClip) - my;
            cxx += xc * xc; cyy += yc * yc; cxy += xc * yc;
        }
        acc += cxy / ((sqrt(cxx) + kStoiEps) * (sqrt(cyy) + kStoiEps));
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) L.partial[(size_t)b * L.max_partials + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- 5. merge, one thread per clip ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stoi_finish_kernel(StoiLaunch L) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B) return;
    const int nseg = L.kcount[b] - 1 - (kStoiN - 1);
    if (nseg < 1) { L.out[b] = 1e-5; return; }             // fewer than 30 frames: no 384 ms segment
    const int np = (nseg + kStoiSegChunk - 1) / kStoiSegChunk;
    const double* __restrict__ p = L.partial + (size_t)b * L.max_partials;
    double s = 0.0;
    for (int i = 0; i < np; ++i) s += p[i];
    L.out[b] = s / ((double)nseg * kStoiBands);
}

}  // namespace

void launch_stoi(const StoiLaunch& L, hipStream_t st) {
    const int F = L.max_frames;
    if (F > 0) {
        // a wave takes several frames of a long clip: at most 64 workgroups per clip
        const int gx = std::min((F + kStoiWaves - 1) / kStoiWaves, 64);
        hipLaunchKernelGGL(stoi_energy_kernel, dim3(gx, L.B), dim3(256), 0, st, L);
    }
    hipLaunchKernelGGL(stoi_scan_kernel, dim3(L.B), dim3(256), 0, st, L);
    if (F > 1) hipLaunchKernelGGL(stoi_bands_kernel, dim3((F - 1 + kStoiWaves - 1) / kStoiWaves, L.B), dim3(256), 0, st, L);
    if (F - kStoiN > 0)
        hipLaunchKernelGGL(stoi_segments_kernel, dim3(L.max_partials, L.B), dim3(256), 0, st, L);
    hipLaunchKernelGGL(stoi_finish_kernel, dim3((L.B + 255) / 256), dim3(256), 0, st, L);
}

}  // namespace aware
