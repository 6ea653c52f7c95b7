// Reverberation (EXTENSION, parity unpinned: the reference has neither the attack nor a chain inside its loop): a drawn
// impulse response per clip and the partitioned FFT convolution that applies it.  DESIGN.md section 16; the torch
// restatement is aware_amd/embedding/loop_attacks.py::reverb_ir / apply_chain.
//
//   r = philox4x32_10((0, s, 1 + j, 1), (seed_b, 0x5EED)),  on = (r0 + 0.5) / 2^32 < prob,
//   n_h = n_lo + ((r2 * (n_hi - n_lo + 1)) >> 32)
//   t_i = eps_i exp(-ln(1000) i / n_h), 1 <= i < n_h, eps_i from philox((i / 4, s, 8, j), (seed_b, 0x5EED)), Box-Muller
//   h_0 = 10^(drr_db / 20) sqrt(sum t_i^2),  h_i = t_i
//   forward   z = (h * x)[0 : Ny]                 adjoint   gx[i] = sum_k h_k gy[i + k]
//
// Overlap-save on 4096-point transforms, one wave per transform (fft_any.hpp, M = 2048): the signal in blocks of 4096
// samples advancing by 2048, the response in up to four partitions of 2048 taps.  Output block k is
//   irfft(sum_p X_{k-p} H_p)[2048 : 4096]   with X_k = rfft(x[2048 (k - 1) : 2048 (k + 1)]),   and for the adjoint
//   irfft(sum_p G_{k+p} conj(H_p))[0 : 2048] with G_k = rfft(gy[2048 k : 2048 (k + 2)]);
// the signal is zero outside [0, Ny).  Four kernels, nothing atomic, every sum in a fixed order:
//   reverb_ir_kernel     one workgroup per clip: the draw, the tail, sum t^2 in f64, h and n_h
//   spectra_kernel<H>    one wave per (clip, partition) / per (clip, block): the spectra, the only scratch
//   apply_kernel         one wave per (clip, output block): the sum over the partitions and the inverse transform
// A clip whose entry does not fire (n_h = 0) is copied: the identity is exact.
#include "common.hpp"
#include "fft_any.hpp"
#include "kernels.h"
#include "loop_stage.hpp"

namespace aware {

namespace {

constexpr int kRvM = kReverbBlock;          // complex points of the packed transform
constexpr int kRvS = kRvM + 8;              // LDS row and spectrum row (kReverbBins)
constexpr int kRvWaves = 4;
static_assert(kRvS == kReverbBins && kReverbTwHalf == kRvM / 2 && kReverbParts * kReverbBlock == kReverbMaxIr, "");

__global__ __launch_bounds__(256) void reverb_ir_kernel(ReverbIrLaunch a) {
    __shared__ double dred[4];
    const int b = blockIdx.x;
    if (loop_gate_skips(a.gate, b)) return;
    const unsigned step = (unsigned)(a.step ? *a.step : a.step_imm), seed = a.seeds[b], j = (unsigned)a.entry;
    unsigned r[4];
    philox4x32_10(0u, step, 1u + j, 1u, seed, 0x5EEDu, r);
    const bool on = loop_entry_fires(r[0], a.prob);
    const int n_h = loop_uniform(r[2], a.n_lo, a.n_hi);
    float* h = a.h + (size_t)b * a.h_stride;
    const double rate = -6.907755278982137 / (double)n_h;       // -ln(1000) / n_h
    double acc = 0.0;
    for (int q = threadIdx.x; 4 * q < a.h_stride; q += 256) {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        if (on && 4 * q < n_h) {
            float eps[4];
            normal4w((unsigned)q, step, 8u, j, seed, eps);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = 4 * q + e;
                if (i >= 1 && i < n_h) {
                    t[e] = (float)((double)eps[e] * exp(rate * (double)i));
                    acc += (double)t[e] * (double)t[e];
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * q + e < a.h_stride) h[4 * q + e] = t[e];
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) dred[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        h[0] = on ? (float)(a.gain * sqrt(dred[0] + dred[1] + dred[2] + dred[3])) : 1.f;
        a.nh[b] = on ? n_h : 0;
    }
}

struct ClipSpan { int off, n; };
__device__ __forceinline__ ClipSpan clip_span(const ConvolveLaunch& a, int b) {
    ClipSpan c;
    if (a.off) { c.off = a.off[b]; c.n = a.len[b]; }
    else { c.off = sig_offset(a.frame_off, b); c.n = kHop * (a.frame_off[b + 1] - a.frame_off[b] - 1); }
    return c;
}

__device__ __forceinline__ void load_tables(cf* th, const cf* src) {
    for (int i = threadIdx.x; i < kRvM / 2; i += blockDim.x) th[i] = src[i];
    __syncthreads();
}

// IS_H: wave p of workgroup b transforms taps [2048 p, 2048 (p + 1)) of clip b's response, zero-padded to 4096;
// else wave k transforms the 4096 samples around block k of clip b's signal
template <bool IS_H>
__global__ __launch_bounds__(256) void spectra_kernel(ConvolveLaunch a) {
    __shared__ cf sbuf[kRvWaves][kRvS];
    __shared__ cf th[kRvM / 2];
    if (loop_gate_skips(a.gate, blockIdx.y)) return;        // the whole workgroup: in front of the barrier
    load_tables(th, a.tables);
    const cf* twN = a.tables + kReverbTwHalf;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y, k = blockIdx.x * kRvWaves + wv;
    const int nh = min(a.nh[b], min(a.h_stride, a.parts * kReverbBlock));
    if (nh <= 0) return;
    const float* x;
    int base, n;
    cf* row;
    if (IS_H) {
        if (k >= a.parts || k * kReverbBlock >= nh) return;
        x = a.h + (size_t)b * a.h_stride;
        base = k * kReverbBlock;
        n = min(nh, base + kReverbBlock);
        row = a.hspec + ((size_t)b * a.parts + k) * kRvS;
    } else {
        const ClipSpan c = clip_span(a, b);
        if (k >= a.kmax || k * kReverbBlock >= c.n) return;
        x = a.in + c.off;
        base = a.adjoint ? k * kReverbBlock : (k - 1) * kReverbBlock;
        n = c.n;
        row = a.xspec + ((size_t)b * a.kmax + k) * kRvS;
    }
    cf* s = sbuf[wv];
#pragma unroll 4
    for (int i = 0; i < kRvM / 128; ++i) {
        const int q = lane + 64 * i;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = base + 4 * q + e;
            v[e] = (idx >= 0 && idx < n) ? x[idx] : 0.f;
        }
        s[2 * q] = mk(v[0], v[1]);
        s[2 * q + 1] = mk(v[2], v[3]);
    }
    wave_sync();
    fa::fft_wave<kRvM, -1>(lane, s, th);
    float4* row4 = reinterpret_cast<float4*>(row);
#pragma unroll 4
    for (int i = 0; i <= kRvM / 128; ++i) {
        const int q = lane + 64 * i;
        if (q >= kRvS / 2) break;
        cf X[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int kk = 2 * q + e;
            X[e] = kk <= kRvM ? fa::rfft_bin<kRvM>(kk, s, twN) : mk(0.f, 0.f);
        }
        row4[q] = make_float4(X[0].x, X[0].y, X[1].x, X[1].y);
    }
}

// s[0 .. 2056) = sum over p < P of X_{k-p} H_p (adjoint: X_{k+p} conj(H_p)), ascending p.  The loads of a pair of bins do not
// depend on anything computed here, so with P fixed at compile time the compiler issues those of several pairs ahead of
// the sums; a term whose block lies outside the clip loads a row that exists and counts as zero.
template <int P>
__device__ __forceinline__ void accumulate(int lane, int adjoint, int k, int K, const cf* hs, const cf* xs, cf* s) {
    const float4* xr[P];
    const float4* hr[P];
    float w[P];
    const float sgn = adjoint ? -1.f : 1.f;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int kp = adjoint ? k + p : k - p;
        const bool ok = kp >= 0 && kp < K;
        w[p] = ok ? 1.f : 0.f;
        xr[p] = reinterpret_cast<const float4*>(xs + (size_t)(ok ? kp : k) * kRvS);
        hr[p] = reinterpret_cast<const float4*>(hs + (size_t)p * kRvS);
    }
    constexpr int kUnroll = P <= 2 ? 4 : 2;
#pragma unroll kUnroll
    for (int i = 0; i <= kRvM / 128; ++i) {
        const int q = lane + 64 * i;
        if (q >= kRvS / 2) break;
        float4 xv[P], hv[P];
#pragma unroll
        for (int p = 0; p < P; ++p) { xv[p] = xr[p][q]; hv[p] = hr[p][q]; }
        cf acc0 = mk(0.f, 0.f), acc1 = mk(0.f, 0.f);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            acc0 = acc0 + cmul(mk(xv[p].x * w[p], xv[p].y * w[p]), mk(hv[p].x, hv[p].y * sgn));
            acc1 = acc1 + cmul(mk(xv[p].z * w[p], xv[p].w * w[p]), mk(hv[p].z, hv[p].w * sgn));
        }
        if (2 * q == 0 || 2 * q == kRvM) acc0.y = 0.f;      // irfft ignores the imaginary parts of DC and Nyquist
        s[2 * q] = acc0;
        s[2 * q + 1] = acc1;
    }
}

__global__ __launch_bounds__(256) void apply_kernel(ConvolveLaunch a) {
    __shared__ cf sbuf[kRvWaves][kRvS];
    __shared__ cf th[kRvM / 2];
    if (loop_gate_skips(a.gate, blockIdx.y)) return;        // the whole workgroup: in front of the barrier
    load_tables(th, a.tables);
    const cf* twN = a.tables + kReverbTwHalf;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y, k = blockIdx.x * kRvWaves + wv;
    const ClipSpan c = clip_span(a, b);
    if (k >= a.kmax || k * kReverbBlock >= c.n) return;
    const int o0 = k * kReverbBlock;
    float* out = a.out + c.off + o0;
    const int nh = min(a.nh[b], min(a.h_stride, a.parts * kReverbBlock));
    if (nh <= 0) {
        // the entry does not fire: the identity, exactly
        const float* in = a.in + c.off + o0;
        if (in != out)
            for (int t = lane; t < kReverbBlock && o0 + t < c.n; t += 64) out[t] = in[t];
        return;
    }
    const int P = (nh + kReverbBlock - 1) / kReverbBlock, K = min((c.n + kReverbBlock - 1) / kReverbBlock, a.kmax);
    cf* s = sbuf[wv];
    const cf* hs = a.hspec + (size_t)b * a.parts * kRvS;
    const cf* xs = a.xspec + (size_t)b * a.kmax * kRvS;
    switch (P) {
        case 1: accumulate<1>(lane, a.adjoint, k, K, hs, xs, s); break;
        case 2: accumulate<2>(lane, a.adjoint, k, K, hs, xs, s); break;
        case 3: accumulate<3>(lane, a.adjoint, k, K, hs, xs, s); break;
        default: accumulate<4>(lane, a.adjoint, k, K, hs, xs, s); break;
    }
    wave_sync();
    fa::irfft_merge_lane<kRvM>(lane, s, twN);
    wave_sync();
    fa::fft_wave<kRvM, 1>(lane, s, th);
    // s[m] / M = y[2m] + i y[2m + 1] of the 4096-point result: its second half (forward) or its first (adjoint)
    const cf* res = s + (a.adjoint ? 0 : kRvM / 2);
    const float sc = 1.0f / (float)kRvM;
#pragma unroll 4
    for (int i = 0; i < kRvM / 128; ++i) {
        const int m = lane + 64 * i;
        const cf v = res[m];
        if (o0 + 2 * m < c.n) out[2 * m] = v.x * sc;
        if (o0 + 2 * m + 1 < c.n) out[2 * m + 1] = v.y * sc;
    }
}

}  // namespace

void launch_reverb_ir(const ReverbIrLaunch& L, hipStream_t st) {
    hipLaunchKernelGGL(reverb_ir_kernel, dim3((unsigned)L.B), dim3(256), 0, st, L);
}

void launch_convolve(const ConvolveLaunch& L, hipStream_t st) {
    const dim3 grid((unsigned)((L.kmax + kRvWaves - 1) / kRvWaves), (unsigned)L.B, 1);
    if (!L.skip_h) hipLaunchKernelGGL(spectra_kernel<true>, dim3(1, (unsigned)L.B, 1), dim3(256), 0, st, L);
    hipLaunchKernelGGL(spectra_kernel<false>, grid, dim3(256), 0, st, L);
    hipLaunchKernelGGL(apply_kernel, grid, dim3(256), 0, st, L);
}

}  // namespace aware
