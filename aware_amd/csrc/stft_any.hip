// The general-geometry STFT path: torch.stft / torch.istft (center=True, reflect padding, one-sided) for any n_fft in
// {256, 512, 1024, 2048, 4096}, any hop in 1..n_fft and any win_length in 1..n_fft (reference: utils/audio/stft.py:14-48),
// with the adjoints of both for the plug-ins' backward.  The card geometry keeps its own kernels (dsp_kernels.hip,
// dsp_stream.hip).
//
// Layout: one wave transforms one frame (fft_any.hpp); a 256-thread workgroup holds four frames and one copy of the
// twiddle half-table in LDS.  Spectrum rows are read and written as 16-byte vectors.  The synthesis direction writes its
// windowed frames to the batch's frame buffer and a second kernel overlap-adds them per output sample (the overlap is
// served from L2 / the infinity cache instead of an LDS chunk; the hop is a runtime value).
#include <hip/hip_runtime.h>
#include "common.hpp"
#include "fft_any.hpp"
#include "kernels.h"

namespace aware {
namespace {

constexpr int kGenWaves = 4;

// clip of global frame f: frame_off[b] <= f < frame_off[b + 1] (binary search, the same for all lanes)
__device__ __forceinline__ int clip_of_frame(const int* frame_off, int B, int f) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (frame_off[mid] <= f) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void load_half_table(cf* th, const cf* src, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) th[i] = src[i];
    __syncthreads();
}

// ---- analysis: frame -> window -> rFFT -> row ---------------------------------------------------------------------
template <int M, int ADJ>
__global__ __launch_bounds__(256) void gen_analysis_kernel(GenLaunch L, const float* __restrict__ sig, cf* __restrict__ spec) {
    constexpr int N = 2 * M, S = M + 8;
    __shared__ cf sbuf[kGenWaves][S];
    __shared__ cf th[M / 2];
    load_half_table(th, L.plan.th, M / 2);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int f = blockIdx.x * kGenWaves + wv;
    if (f >= L.NF) return;
    cf* s = sbuf[wv];
    const int b = clip_of_frame(L.frame_off, L.B, f);
    const int t = f - L.frame_off[b], T = L.frame_off[b + 1] - L.frame_off[b];
    const int hop = L.plan.hop;
    const float* __restrict__ w = L.plan.window;
    const int base = t * hop - N / 2;          // signal index of frame sample 0 (before the reflection)
    if (!ADJ) {
        const int n = L.sig_len[b];
        const float* x = sig + L.sig_off[b];
        float inv = 1.f;
        if (L.pmax) {
            unsigned long long v = 0;
            const unsigned long long* part = L.pmax + (size_t)b * L.pstride;
            for (int i = lane; i < L.pcount[b]; i += 64) v = umax64(v, part[i]);
            v = wave_max64(v);
            inv = 1.0f / (__uint_as_float((unsigned)(v >> 32)) + 1e-8f);
        }
#pragma unroll
        for (int i = 0; i < M / 128; ++i) {
            const int q = lane + 64 * i;
            float r[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int o = 4 * q + e;
                const float wo = w[o];
                int idx = base + o;
                idx = idx < 0 ? -idx : idx;
                idx = idx >= n ? 2 * (n - 1) - idx : idx;
                // n > n_fft/2 (every clip aware_stft takes): in range already.  The embed loop's second analysis reads the
                // synthesis, hop (T - 1) samples, which may be n_fft/2 or fewer; torch.stft refuses to pad such a signal
                idx = min(max(idx, 0), n - 1);
                r[e] = wo != 0.f ? (x[idx] * inv) * wo : 0.f;
            }
            s[2 * q] = mk(r[0], r[1]);
            s[2 * q + 1] = mk(r[2], r[3]);
        }
    } else {
        // d loss / d frame_t[o] = w[o] g[p - N/2] / env(p) at p = t hop + o inside the trimmed output, else 0
        const int len = L.out_len[b];
        const float* g = sig + L.out_off[b];
#pragma unroll
        for (int i = 0; i < M / 128; ++i) {
            const int q = lane + 64 * i;
            float r[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int o = 4 * q + e;
                const int idx = base + o;
                const float wo = w[o];
                r[e] = 0.f;
                if (wo != 0.f && idx >= 0 && idx < len)
                    r[e] = wo * (g[idx] / gen_env(L.plan.env, L.plan.window2, N, hop, idx + N / 2, T));
            }
            s[2 * q] = mk(r[0], r[1]);
            s[2 * q + 1] = mk(r[2], r[3]);
        }
    }
    wave_sync();
    fa::fft_wave<M, -1>(lane, s, th);
    // bins k = 0..M; the row's padding columns are written as zero.  irfft's adjoint weighs bin k by c_k / N
    // (c = 1 at DC and Nyquist, 2 in between).
    const cf* twN = L.plan.twN;
    float4* row = reinterpret_cast<float4*>(spec + (size_t)f * S);
#pragma unroll
    for (int i = 0; i <= M / 128; ++i) {
        const int q = lane + 64 * i;
        if (q >= S / 2) break;
        cf X[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int k = 2 * q + e;
            X[e] = mk(0.f, 0.f);
            if (k <= M) {
                X[e] = fa::rfft_bin<M>(k, s, twN);
                if (ADJ) {
                    const float c = (k == 0 || k == M) ? 1.0f / N : 2.0f / N;
                    X[e] = mk(X[e].x * c, X[e].y * c);
                }
            }
        }
        row[q] = make_float4(X[0].x, X[0].y, X[1].x, X[1].y);
    }
}

// ---- synthesis, part 1: row -> irFFT -> window -> frame buffer -----------------------------------------------------
template <int M, int ADJ>
__global__ __launch_bounds__(256) void gen_frames_kernel(GenLaunch L, const cf* __restrict__ spec) {
    constexpr int N = 2 * M, S = M + 8;
    __shared__ cf sbuf[kGenWaves][S];
    __shared__ cf th[M / 2];
    load_half_table(th, L.plan.th, M / 2);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int f = blockIdx.x * kGenWaves + wv;
    if (f >= L.NF) return;
    cf* s = sbuf[wv];
    // irfft ignores the imaginary parts of DC and Nyquist.  The adjoint of the analysis is N * irfft of the cotangent
    // with the bins strictly between DC and Nyquist halved.
    const float4* row = reinterpret_cast<const float4*>(spec + (size_t)f * S);
#pragma unroll
    for (int i = 0; i <= M / 128; ++i) {
        const int q = lane + 64 * i;
        if (q >= S / 2) break;
        const float4 v = row[q];
        cf a = mk(v.x, v.y), c = mk(v.z, v.w);
        if (2 * q == 0 || 2 * q == M) a.y = 0.f;
        if (ADJ) {
            if (2 * q != 0 && 2 * q != M) a = mk(0.5f * a.x, 0.5f * a.y);
            if (2 * q + 1 != M) c = mk(0.5f * c.x, 0.5f * c.y);
        }
        s[2 * q] = a;
        s[2 * q + 1] = c;
    }
    wave_sync();
    fa::irfft_merge_lane<M>(lane, s, L.plan.twN);
    wave_sync();
    fa::fft_wave<M, 1>(lane, s, th);
    const float* __restrict__ w = L.plan.window;
    const float sc = ADJ ? (float)N / (float)M : 1.0f / (float)M;
    float4* out = reinterpret_cast<float4*>(L.frames + (size_t)f * N);
#pragma unroll
    for (int i = 0; i < M / 128; ++i) {
        const int q = lane + 64 * i;
        const cf a = s[2 * q], c = s[2 * q + 1];
        const float4 wv4 = reinterpret_cast<const float4*>(w)[q];
        out[q] = make_float4((a.x * sc) * wv4.x, (a.y * sc) * wv4.y, (c.x * sc) * wv4.z, (c.y * sc) * wv4.w);
    }
}

// sum_t frames[f0 + t][p - hop t] over the frames of a T-frame clip that cover padded position p (ascending t)
__device__ __forceinline__ float ola_sum(const float* __restrict__ fr, int N, int hop, int p, int T) {
    const int tlo = p - N + 1 > 0 ? (p - N + hop) / hop : 0;
    const int thi = (p / hop < T - 1) ? p / hop : T - 1;
    float acc = 0.f;
    for (int t = tlo; t <= thi; ++t) acc += fr[(size_t)t * N + p - hop * t];
    return acc;
}

// ---- synthesis, part 2: overlap-add per output sample --------------------------------------------------------------
template <int ADJ>
__global__ __launch_bounds__(256) void gen_ola_kernel(GenLaunch L, float* __restrict__ out) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int N = L.plan.n_fft, hop = L.plan.hop;
    const int f0 = L.frame_off[b], T = L.frame_off[b + 1] - f0;
    const float* fr = L.frames + (size_t)f0 * N;
    if (!ADJ) {
        if (i >= L.out_len[b]) return;
        const int p = i + N / 2;
        out[L.out_off[b] + i] = ola_sum(fr, N, hop, p, T) / gen_env(L.plan.env, L.plan.window2, N, hop, p, T);
    } else {
        // x[i] feeds padded positions i + N/2 and its reflections N/2 - i (1 <= i <= N/2) and N/2 + 2n - 2 - i
        // (n - 1 - N/2 <= i <= n - 2)
        const int n = L.sig_len[b];
        if (i >= n) return;
        float g = ola_sum(fr, N, hop, i + N / 2, T);
        if (i >= 1 && i <= N / 2) g += ola_sum(fr, N, hop, N / 2 - i, T);
        if (i >= n - 1 - N / 2 && i <= n - 2) g += ola_sum(fr, N, hop, N / 2 + 2 * n - 2 - i, T);
        out[L.sig_off[b] + i] = g;
    }
}

__global__ __launch_bounds__(256) void gen_normalize_kernel(GenLaunch L, float* __restrict__ out) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= L.out_len[b]) return;
    unsigned long long v = 0;
    const unsigned long long* part = L.pmax + (size_t)b * L.pstride;
    for (int k = 0; k < L.pcount[b]; ++k) v = umax64(v, part[k]);
    const float m = __uint_as_float((unsigned)(v >> 32)) + 1e-8f;
    out[L.out_off[b] + i] = out[L.out_off[b] + i] / m;
}

template <int M>
void analysis_m(const GenLaunch& L, const float* sig, void* spec, int adjoint, hipStream_t st) {
    const dim3 grid((L.NF + kGenWaves - 1) / kGenWaves);
    if (adjoint) hipLaunchKernelGGL((gen_analysis_kernel<M, 1>), grid, dim3(256), 0, st, L, sig, (cf*)spec);
    else hipLaunchKernelGGL((gen_analysis_kernel<M, 0>), grid, dim3(256), 0, st, L, sig, (cf*)spec);
}
template <int M>
void frames_m(const GenLaunch& L, const void* spec, int adjoint, hipStream_t st) {
    const dim3 grid((L.NF + kGenWaves - 1) / kGenWaves);
    if (adjoint) hipLaunchKernelGGL((gen_frames_kernel<M, 1>), grid, dim3(256), 0, st, L, (const cf*)spec);
    else hipLaunchKernelGGL((gen_frames_kernel<M, 0>), grid, dim3(256), 0, st, L, (const cf*)spec);
}

}  // namespace

void launch_gen_analysis(const GenLaunch& L, const float* sig, void* spec, int adjoint, hipStream_t st) {
    switch (L.plan.n_fft) {
        case 256: analysis_m<128>(L, sig, spec, adjoint, st); break;
        case 512: analysis_m<256>(L, sig, spec, adjoint, st); break;
        case 1024: analysis_m<512>(L, sig, spec, adjoint, st); break;
        case 2048: analysis_m<1024>(L, sig, spec, adjoint, st); break;
        default: analysis_m<2048>(L, sig, spec, adjoint, st); break;
    }
}

void launch_gen_synthesis(const GenLaunch& L, const void* spec, float* out, int adjoint, hipStream_t st) {
    switch (L.plan.n_fft) {
        case 256: frames_m<128>(L, spec, adjoint, st); break;
        case 512: frames_m<256>(L, spec, adjoint, st); break;
        case 1024: frames_m<512>(L, spec, adjoint, st); break;
        case 2048: frames_m<1024>(L, spec, adjoint, st); break;
        default: frames_m<2048>(L, spec, adjoint, st); break;
    }
    const dim3 grid((L.max_len + 255) / 256, L.B);
    if (adjoint) hipLaunchKernelGGL(gen_ola_kernel<1>, grid, dim3(256), 0, st, L, out);
    else hipLaunchKernelGGL(gen_ola_kernel<0>, grid, dim3(256), 0, st, L, out);
}

void launch_gen_normalize(const GenLaunch& L, float* out, hipStream_t st) {
    const dim3 grid((L.max_len + 255) / 256, L.B);
    hipLaunchKernelGGL(gen_normalize_kernel, grid, dim3(256), 0, st, L, out);
}

}  // namespace aware
