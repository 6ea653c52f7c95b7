// The detector's mel stage, stated once: InstanceNorm1d over time (biased variance, eps 1e-5) -> GlobalStandardize per clip
// (unbiased std, eps 1e-8) -> AvgPool1d(2, 2), and the backward of the three.  The kernels that run it -- the chunked family
// and the clip kernels of detector_kernels.hip, mel_front_x3_kernel and mel_back_x3_kernel of gemm_x3.hip -- differ in how
// they hold the clip's rows and reduce over them; every scalar expression is written here, once.
//
// With u = (x - mu_c) * rs_c the per-channel sums are  sum_t u = 0  and  sum_t u^2 = rs_c^2 * M2_c  exactly, so the clip-wide
// mean of u is taken as 0 (the reference evaluates a rounding residue of order 1e-9 there, globalStandardize.py:17) and its
// unbiased std follows from the per-channel M2.
//   stats[b][c] = {mu, rs, M2, 0}   (rows of Mp channels per clip; padding channels hold zeros)
//   gstat[b]    = {1 / (gs + 1e-8), gs, n, T}   with n = T * n_mels
// The expression trees (parentheses, constants, operand order) and the shape of the helpers (values in, values out: an
// accumulator passed by reference fused the other product of mel_dv_u) decide how the compiler contracts them into FMAs, and a
// kernel that packs a frame pair into one two-lane multiply (the 128-band clip forward, mel_front_x3_kernel) rounds both
// products of mel_pooled where the others fuse one.  tests/test_gpu_mel_norm_bits.py holds the bits of every kernel: run it
// after any change here or to the code around a call.
#pragma once
#include <hip/hip_runtime.h>

namespace aware {

constexpr int kMelChunk = 32;                       // frames per chunk of the chunked form

struct MelChan { float mu, rs, M2; };               // InstanceNorm statistics of one channel of one clip
struct MelClip { float ginv, gs, n; };              // GlobalStandardize of one clip
struct MelClipGrad { float mdv, Q; };               // the backward's clip-wide terms
struct MelChanGrad { float m1, m2; };               // the backward's per-channel terms

__device__ __forceinline__ float mel_rs(float M2, float T) { return 1.0f / sqrtf(M2 / T + 1e-5f); }
// a channel's share of the clip's sum of u^2
__device__ __forceinline__ float mel_suu(float rs, float M2) { return rs * rs * M2; }
__device__ __forceinline__ MelClip mel_clip(float suu, float T, int n_mels) {
    MelClip k;
    k.n = T * (float)n_mels;
    k.gs = sqrtf(suu / (k.n - 1.f));                // unbiased std of u (mean 0)
    k.ginv = 1.0f / (k.gs + 1e-8f);
    return k;
}

// i: the channel's index b * Mp + ch
__device__ __forceinline__ void mel_write_stats(float* __restrict__ stats, size_t i, float mu, float rs, float M2) {
    float* st = stats + i * 4;
    st[0] = mu; st[1] = rs; st[2] = M2; st[3] = 0.f;
}
__device__ __forceinline__ MelChan mel_read_stats(const float* __restrict__ stats, size_t i) {
    const float* st = stats + i * 4;
    return MelChan{st[0], st[1], st[2]};
}
__device__ __forceinline__ void mel_write_gstat(float* __restrict__ gstat, int b, const MelClip& k, float T) {
    gstat[b * 4 + 0] = k.ginv; gstat[b * 4 + 1] = k.gs; gstat[b * 4 + 2] = k.n; gstat[b * 4 + 3] = T;
}
__device__ __forceinline__ MelClip mel_read_gstat(const float* __restrict__ gstat, int b) {
    return MelClip{gstat[b * 4 + 0], gstat[b * 4 + 1], gstat[b * 4 + 2]};
}

__device__ __forceinline__ float mel_u(float x, float mu, float rs) { return (x - mu) * rs; }
// AvgPool1d(2, 2) of the standardised frame pair
__device__ __forceinline__ float mel_pooled(float u0, float u1, float ginv) { return 0.5f * (u0 * ginv + u1 * ginv); }

// backward.  dv: dL/d(standardised frame) = half the pooled gradient on both frames of a pair (0 on an unpaired last frame);
// a frame pair's share of D2_c = sum_t dv * u (its share of D1_c = sum_t dv is 2 dv)
__device__ __forceinline__ float mel_dv_u(float dv, float u0, float u1) { return dv * u0 + dv * u1; }
// sa, sb: D1 and D2 summed over the clip's channels
__device__ __forceinline__ MelClipGrad mel_clip_grad(float sa, float sb, const MelClip& k) {
    MelClipGrad q;
    q.mdv = sa / k.n;
    q.Q = (k.gs > 0.f) ? sb * k.ginv * k.ginv / ((k.n - 1.f) * k.gs) : 0.f;
    return q;
}
__device__ __forceinline__ MelChanGrad mel_chan_grad(float D1, float D2, float T, float rs, float M2, const MelClip& k,
                                                     const MelClipGrad& q) {
    MelChanGrad m;
    m.m1 = k.ginv * (D1 / T - q.mdv);
    m.m2 = (k.ginv * D2 - q.Q * rs * rs * M2) / T;
    return m;
}
// dL/dx of one frame of one channel
__device__ __forceinline__ float mel_bwd_value(float dv, float u, float rs, float ginv, const MelClipGrad& q,
                                               const MelChanGrad& m) {
    return rs * (((dv - q.mdv) * ginv - u * q.Q) - m.m1 - u * m.m2);
}

// the partial sums of a workgroup's eight waves, in the one order every kernel uses
__device__ __forceinline__ float mel_sum8(const float* r) { return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])); }

// Chan's merge of the chunk partials {mean, M2} of channel ch, chunks in order; part: the clip's rows [chunk][2 Mp]
// (all threads with the same ch get the same result)
__device__ __forceinline__ void mel_merge(const float* __restrict__ part, int nchunk, int T, int ch, int Mp, float& mean,
                                          float& M2) {
    float n = 0.f;
    mean = 0.f; M2 = 0.f;
    for (int k = 0; k < nchunk; ++k) {
        const float nk = (float)min(kMelChunk, T - k * kMelChunk);
        const float mk = part[(size_t)k * 2 * Mp + ch], qk = part[(size_t)k * 2 * Mp + Mp + ch];
        const float d = mk - mean, nn = n + nk;
        mean += d * (nk / nn);
        M2 += qk + d * d * (n * nk / nn);
        n = nn;
    }
}

}  // namespace aware
