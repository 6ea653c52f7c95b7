// The gain envelope of the embed loop's attack chains (chain kind 8; EXTENSION): what the stage kernels
// (loop_attack_kernels.hip) and the stand-alone entry (loop_gain_kernels.hip) share.  The host twin is
// aware_amd/embedding/loop_attacks.py::envelope_draw / envelope_gains / envelope_curve.
//
//   r = philox4x32_10((0, s, 1 + j, 1), (seed_b, 0x5EED));  P = P_lo + ((r2 * (P_hi - P_lo + 1)) >> 32),  ph = (r1 * P) >> 32
//   breakpoint k:  w_k = philox4x32_10((k / 4, s, 16 + j, 0), (seed_b, 0x5EED))[k % 4],  g_k = floor + (1 - floor) (w_k >> 8) 2^-24
//   sample i:      pos = i + ph,  k = pos / P,  f = (pos - k P) / P,  g(i) = g_k + f (g_{k+1} - g_k)
//
// A workgroup works on at most kEnvSpan consecutive samples of one clip, so it meets at most kEnvSpan / 64 + 2 breakpoints per
// entry: it draws them once into a table in LDS (one Philox call per four, from the quad that holds the first) and then finds
// k and f of a sample from the distance to the workgroup's first sample -- below 2^21, so a float reciprocal and one
// correction step give the exact quotient, with no integer division per sample.
#pragma once
#include "common.hpp"
#include "loop_stage.hpp"

namespace aware {

constexpr int kEnvSpan = kSynthBlocks * kHop;                              // samples per workgroup, at most
constexpr int kEnvTab = kEnvSpan / kEnvelopeMinPeriod + 8;                 // table entries: 3 of the quad in front, span / P + 3 met
constexpr int kEnvQuads = kEnvTab / 4;
constexpr unsigned kEnvWord = 16u;                                         // third Philox counter word of entry j: 16 + j
static_assert(kEnvTab % 4 == 0 && kEnvQuads <= 64, "one Philox call per quad, by the first wave");

// one entry's envelope on one workgroup's samples; uniform over the workgroup
struct EnvBlock {
    int P;          // samples between breakpoints
    float invP;
    int rb;         // (first sample + ph) % P
    int tb;         // table index of the breakpoint at or in front of the first sample (0..3)
};

// P and ph of the entry from its draw r
__device__ __forceinline__ void envelope_draw(const unsigned (&r)[4], int p_lo, int p_hi, int& P, int& ph) {
    P = loop_uniform(r[2], p_lo, p_hi);
    ph = loop_below(r[1], P);
}

// The table of the workgroup whose first sample is i_first (< 2^31): the threads below kEnvQuads draw four breakpoints each.
// The caller synchronises the workgroup before it reads the table.
__device__ __forceinline__ EnvBlock envelope_block(float* tab, int i_first, int P, int ph, float floor, unsigned step, unsigned j,
                                                   unsigned seed) {
    const unsigned pos = (unsigned)i_first + (unsigned)ph;                 // < 2^31 + 2^20
    const unsigned kb = pos / (unsigned)P;
    EnvBlock eb;
    eb.P = P; eb.invP = 1.0f / (float)P; eb.rb = (int)(pos - kb * (unsigned)P); eb.tb = (int)(kb & 3u);
    if (threadIdx.x < kEnvQuads) {
        unsigned w[4];
        philox4x32_10((kb >> 2) + threadIdx.x, step, kEnvWord + j, 0u, seed, 0x5EEDu, w);
#pragma unroll
        for (int e = 0; e < 4; ++e) tab[4 * threadIdx.x + e] = floor + (1.0f - floor) * ((float)(w[e] >> 8) * 5.9604644775390625e-08f);
    }
    return eb;
}

// breakpoint (relative to the workgroup's first) and remainder of the sample d = i - i_first >= 0, d < kEnvSpan
__device__ __forceinline__ void envelope_locate(const EnvBlock& eb, int d, int& kl, int& rem) {
    d += eb.rb;                                                            // < kEnvSpan + 2^20: exact in f32
    kl = (int)((float)d * eb.invP);
    rem = d - kl * eb.P;
    if (rem < 0) { --kl; rem += eb.P; }
    if (rem >= eb.P) { ++kl; rem -= eb.P; }
}
// g at breakpoint kl, remainder rem < P
__device__ __forceinline__ float envelope_gain(const EnvBlock& eb, const float* tab, int kl, int rem) {
    const int t = min(eb.tb + kl, kEnvTab - 2);
    const float ga = tab[t], gb = tab[t + 1];
    return fmaf((float)rem * eb.invP, gb - ga, ga);
}
// g of the four samples from d on
__device__ __forceinline__ void envelope_gain4(const EnvBlock& eb, const float* tab, int d, float (&g)[4]) {
    int kl, rem;
    envelope_locate(eb, d, kl, rem);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool wrap = rem + e >= eb.P;                                 // P >= 64: at most one breakpoint inside
        g[e] = envelope_gain(eb, tab, kl + (wrap ? 1 : 0), rem + e - (wrap ? eb.P : 0));
    }
}

}  // namespace aware
