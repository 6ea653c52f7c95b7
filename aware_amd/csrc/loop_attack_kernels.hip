// Attack-aware embedding (EXTENSION, parity unpinned: the reference optimises against the clean synthesis only): a chain of
// up to four attacks between the synthesis and the analysis of the embed loop, so that the optimiser sees what an attacker
// does to the signal.  DESIGN.md section 15; the torch restatement is aware_amd/embedding/loop_attacks.py::apply_chain.
//
//   x = N(N(y))                                    y: the raw synthesis, N(v) = v / (max|v| + 1e-8)
//   for entry j:  r = philox4x32_10((0, s, 1 + j, 1), (seed_b, 0x5EED)),  on = (r0 + 0.5) / 2^32 < prob_j
//     sample suppression (k samples):  start = (r1 * (Ny - k)) >> 32;  on: x[start : start + k] = 0
//     Gaussian noise (snr_db):         sigma = sqrt(mean(x^2) / 10^(snr_db / 10)) (a constant in the backward pass);
//                                      on: x += sigma * eps, eps_i from philox((i / 4, s, 0, j), (seed_b, 0x5EED)), Box-Muller
//     gain envelope (P_lo, P_hi, floor): g(i) piecewise linear between drawn breakpoints P samples apart (loop_gain.hpp);
//                                      on: x[i] *= g(i) (g a constant in the backward pass, which multiplies by it too)
//   z = x; the loop's analysis then runs on z instead of y
//
// s is the optimiser step read from device memory, so a recorded graph replays with fresh draws.  Three kernels, all on the
// partition of a clip into the synthesis runs (the layout of the partial maxima / partial sums the DSP kernels exchange):
//   chain_kernel<false>  per noise entry: f64 partial sums of x^2 in front of it (fixed order, no atomics)
//   chain_kernel<true>   z and the partial maxima of |z|
//   chain_bwd_kernel     the synthesis adjoint's gradient with respect to N(N(z)) -> the gradient with respect to x
// Each has a second instantiation (ENV) for the stages that hold a gain envelope; every other stage launches the first, which
// holds no code and no LDS of the envelope.
#include "common.hpp"
#include "kernels.h"
#include "loop_gain.hpp"
#include "loop_stage.hpp"

namespace aware {

namespace {

constexpr int kLaThreads = 256;

struct ChainArgs {
    const int* frame_off;                 // [B+1]
    const int* pcount;                    // [B] runs of clip b (= partials per clip)
    int pstride, run_blocks;
    const int* step;                      // device step counter
    int step_back;                        // 1 when the read-out kernel has advanced the counter since the forward pass
    const unsigned* seeds;                // [B]
    int n;                                // chain entries
    int j0;                               // first entry of this stage (0 unless a reverberation or a speed change splits the chain)
    int upto;                             // entries [j0, upto) are applied (sums of squares: those in front of noise entry `upto`)
    const float* src;                     // the stage's input, layout of yraw
    int norm;                             // 1: src is the raw synthesis, x = N(N(src)); 0: src is x itself
    int at_z;                             // chain_bwd_kernel: the stage ends at z (normalisers' backward, reflect pads folded)
    int dot;                              // chain_bwd_kernel: the stage starts at x (partial sums of dL/dx * x)
    int idle_plain;                       // a clip on which no entry fires takes the plain loop's path (chain_idle below)
    float* gpad_out;                      // [B][2][512] with idle_plain: the pads the analysis adjoint reads, per clip
    int kind[kMaxLoopAttacks];
    int k[kMaxLoopAttacks];               // suppression: samples
    double inv_snr[kMaxLoopAttacks];      // noise: 10^(-snr_db / 10)
    float prob[kMaxLoopAttacks];
    int p_lo[kMaxLoopAttacks], p_hi[kMaxLoopAttacks];      // gain envelope: samples between breakpoints, drawn in [p_lo, p_hi]
    float floor[kMaxLoopAttacks];         // gain envelope: the lowest gain
    int B;
    const float* yraw;                    // raw synthesis, clip b at 256 * (frame_off[b] - b)
    const unsigned long long* pmaxY;      // [B][pstride]
    double* psq;                          // [kMaxLoopAttacks][B][pstride] partial sums of x^2 in front of noise entry j
    float* z;                             // as yraw
    unsigned long long* pmaxZ;            // [B][pstride]
    // backward
    float* gy;                            // in: dL/d N(N(z)) (reflect pads folded, or in gpad); out: dL/dx
    float* gdst;                          // where the stage writes dL/dx: gy, or the buffer the speed change's adjoint reads
    const float* gpad;                    // [B][2][512] reflect-pad parts of the streaming synthesis adjoint (null: folded)
    const double* pdot_in;                // [B][pstride] partial sums of gy * N(N(z))
    double* pdot_out;                     // [B][pstride] partial sums of dL/dx * x
    LoopGate gate;                        // inside a mixture: the clips that drew this chain
};

// sum of a clip's f64 partials in a fixed order; all threads of the block call this
__device__ __forceinline__ double block_sum_d(const double* part, int n, double* dred) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kLaThreads) s += part[i];
    s = wave_sum_d(s);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) dred[threadIdx.x >> 6] = s;
    __syncthreads();
    return dred[0] + dred[1] + dred[2] + dred[3];
}

// per-clip state of the chain at this step: which entries fire, where the suppressions start, the noise amplitudes
struct ChainState {
    bool on[kMaxLoopAttacks];
    int start[kMaxLoopAttacks];
    float sigma[kMaxLoopAttacks];
    EnvBlock env[kMaxLoopAttacks];        // gain envelope: its geometry on this workgroup's run (ENV instantiations only)
};
// i_first: the first sample of the workgroup's run; gtab: [kMaxLoopAttacks][kEnvTab] in LDS, complete behind a barrier
template <bool SIGMA, bool ENV>
__device__ __forceinline__ ChainState chain_state(const ChainArgs& a, int b, int j0, int upto, int Ny, unsigned step,
                                                  unsigned seed, double* dred, int i_first = 0, float* gtab = nullptr) {
    ChainState cs;
#pragma unroll
    for (int j = 0; j < kMaxLoopAttacks; ++j) {
        cs.on[j] = false; cs.start[j] = 0; cs.sigma[j] = 0.f;
        if (ENV) cs.env[j] = EnvBlock{kEnvelopeMinPeriod, 0.f, 0, 0};
        if (j >= j0 && j < upto && a.kind[j] != kLoopReverberation && a.kind[j] != kLoopSpeedChange &&
            a.kind[j] != kLoopTimeStretch) {
            unsigned r[4];
            philox4x32_10(0u, step, 1u + (unsigned)j, 1u, seed, 0x5EEDu, r);
            cs.on[j] = loop_entry_fires(r[0], a.prob[j]);
            if (a.kind[j] == kLoopSampleSuppression) {
                cs.start[j] = loop_below(r[1], Ny - a.k[j]);
            } else if (ENV && a.kind[j] == kLoopGainEnvelope) {
                if (cs.on[j]) {
                    int P, ph;
                    envelope_draw(r, a.p_lo[j], a.p_hi[j], P, ph);
                    cs.env[j] = envelope_block(gtab + j * kEnvTab, i_first, P, ph, a.floor[j], step, (unsigned)j, seed);
                }
            } else if (SIGMA) {
                const double ss = block_sum_d(a.psq + ((size_t)j * a.B + b) * a.pstride, a.pcount[b], dred);
                cs.sigma[j] = (float)sqrt(ss / (double)Ny * a.inv_snr[j]);
            }
        }
    }
    if (ENV) __syncthreads();             // the tables are complete
    return cs;
}

// With idle_plain (the chains with a splitting entry or a gain envelope): true when no entry of the whole chain fires for this clip at this step.
// Such a clip is to leave the plain loop's bits.  Forward: z = N(N(y)) as always, but its maxima are recorded as 1 -- what
// max|N(N(y))| is to within an ulp -- so the analysis' two normalisers of z are exactly the identity and it sees the bits the
// plain loop's analysis computes from y.  Backward: the stages hand the synthesis adjoint's gradient, its partial sums
// and its reflect pads through untouched, so the analysis adjoint gets what it gets without a chain.
__device__ __forceinline__ bool chain_idle(const ChainArgs& a, unsigned step, unsigned seed) {
    if (!a.idle_plain) return false;
    bool any = false;
#pragma unroll
    for (int j = 0; j < kMaxLoopAttacks; ++j) {
        if (j < a.n) {
            unsigned r[4];
            philox4x32_10(0u, step, 1u + (unsigned)j, 1u, seed, 0x5EEDu, r);
            any = any || loop_entry_fires(r[0], a.prob[j]);
        }
    }
    return !any;
}

// WRITE = false: partial sums of x^2 with the entries in front of `upto` applied; true: the whole chain, z and max|z|
template <bool WRITE, bool ENV>
__global__ __launch_bounds__(kLaThreads) void chain_kernel(ChainArgs a) {
    __shared__ unsigned long long red[4];
    __shared__ double dred[4];
    __shared__ float gtab[ENV ? kMaxLoopAttacks * kEnvTab : 1];
    const int b = blockIdx.y;
    if (loop_gate_skips(a.gate, b)) return;
    const int nblk = a.frame_off[b + 1] - a.frame_off[b] - 1;
    int nseg, jb0, jb1;
    synth_segment(nblk, blockIdx.x, a.run_blocks, nseg, jb0, jb1);
    if ((int)blockIdx.x >= nseg) return;
    const int Ny = kHop * nblk;
    const int so = sig_offset(a.frame_off, b);
    const ClipNorm cn = clip_norm_from_partials(a.pmaxY + (size_t)b * a.pstride, a.pcount[b], red);
    const float inv_m = a.norm ? 1.0f / cn.m : 1.0f, inv_m2 = a.norm ? 1.0f / cn.m2 : 1.0f;
    const unsigned step = (unsigned)(*a.step - a.step_back), seed = a.seeds[b];
    const ChainState cs = chain_state<true, ENV>(a, b, a.j0, a.upto, Ny, step, seed, dred, jb0 * kHop, gtab);

    const float4* y4 = reinterpret_cast<const float4*>(a.src + so);
    float4* z4 = reinterpret_cast<float4*>(a.z + so);
    unsigned long long best = 0;
    double acc = 0.0;
    for (int q = jb0 * (kHop / 4) + threadIdx.x; q < jb1 * (kHop / 4); q += kLaThreads) {
        const float4 yv = y4[q];
        float v[4] = {(yv.x * inv_m) * inv_m2, (yv.y * inv_m) * inv_m2, (yv.z * inv_m) * inv_m2, (yv.w * inv_m) * inv_m2};
        const int i0 = 4 * q;
#pragma unroll
        for (int j = 0; j < kMaxLoopAttacks; ++j) {
            if (j >= a.j0 && j < a.upto && cs.on[j]) {
                if (a.kind[j] == kLoopSampleSuppression) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if ((unsigned)(i0 + e - cs.start[j]) < (unsigned)a.k[j]) v[e] = 0.f;
                } else if (ENV && a.kind[j] == kLoopGainEnvelope) {
                    float g[4];
                    envelope_gain4(cs.env[j], gtab + j * kEnvTab, i0 - jb0 * kHop, g);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = v[e] * g[e];
                } else {
                    float eps[4];
                    normal4((unsigned)q, step, (unsigned)j, seed, eps);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = v[e] + cs.sigma[j] * eps[e];
                }
            }
        }
        if (WRITE) {
            z4[q] = make_float4(v[0], v[1], v[2], v[3]);
#pragma unroll
            for (int e = 0; e < 4; ++e) best = umax64(best, pack_max(fabsf(v[e]), (unsigned)(i0 + e)));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += (double)v[e] * (double)v[e];
        }
    }
    if (WRITE) {
        best = wave_max64(best);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
        __syncthreads();
        if (threadIdx.x == 0 && a.pmaxZ) {
            unsigned long long m = umax64(umax64(red[0], red[1]), umax64(red[2], red[3]));
            if (chain_idle(a, step, seed)) m = (0x3F800000ull << 32) | (m & 0xFFFFFFFFull);      // max|z| := 1.0f
            a.pmaxZ[(size_t)b * a.pstride + blockIdx.x] = m;
        }
    } else {
        acc = wave_sum_d(acc);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) dred[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) a.psq[((size_t)a.upto * a.B + b) * a.pstride + blockIdx.x] = dred[0] + dred[1] + dred[2] + dred[3];
    }
}

// gy holds G = dL/d N(N(z)) (the synthesis adjoint run on z), pdot_in the partial sums of G * N(N(z)).  Backward of the two
// normalisers at z (scale 1 / (m m2), the arg-max sample also carries -sum * sign(z[k])), identity through the noise (sigma is
// a constant), the 0/1 mask through the suppressions, the gains through the envelopes (all diagonal: their order is free).  The result replaces G; its partial sums against x = N(N(y)) go to
// pdot_out, which is what the analysis adjoint needs for the normalisers in front of the chain.
template <bool ENV>
__global__ __launch_bounds__(kLaThreads) void chain_bwd_kernel(ChainArgs a) {
    __shared__ unsigned long long red[4];
    __shared__ double dred[4];
    __shared__ float gtab[ENV ? kMaxLoopAttacks * kEnvTab : 1];
    const int b = blockIdx.y;
    if (loop_gate_skips(a.gate, b)) return;
    const int nblk = a.frame_off[b + 1] - a.frame_off[b] - 1;
    int nseg, jb0, jb1;
    synth_segment(nblk, blockIdx.x, a.run_blocks, nseg, jb0, jb1);
    if ((int)blockIdx.x >= nseg) return;
    const int Ny = kHop * nblk;
    const int so = sig_offset(a.frame_off, b);
    const ClipNorm cy = clip_norm_from_partials(a.pmaxY + (size_t)b * a.pstride, a.pcount[b], red);
    ClipNorm cz = clip_norm_from_partials(a.pmaxZ + (size_t)b * a.pstride, a.pcount[b], red);
    const float inv_m = 1.0f / cy.m, inv_m2 = 1.0f / cy.m2;
    float inv_mm2 = 1.0f / (cz.m * cz.m2);
    float corr = 0.f;
    if (a.at_z) {
        const float adot = (float)block_sum_d(a.pdot_in + (size_t)b * a.pstride, a.pcount[b], dred);
        const float zk = a.z[so + min(cz.k, (unsigned)(Ny - 1))];
        corr = adot * ((zk > 0.f) ? 1.f : ((zk < 0.f) ? -1.f : 0.f));
    } else {
        cz.k = 0xFFFFFFFFu;                  // a stage in front of the splitting entry: masks and the dot product only
        inv_mm2 = 1.0f;
    }
    const unsigned step = (unsigned)(*a.step - a.step_back), seed = a.seeds[b];
    const bool idle = chain_idle(a, step, seed);
    if (a.dot && a.gpad_out && blockIdx.x == 0) {
        // the pads the analysis adjoint reads: folded into gy already (zeros), or the synthesis adjoint's own for an idle clip
        float* po = a.gpad_out + (size_t)b * 1024;
        const float* pi = (idle && a.gpad) ? a.gpad + (size_t)b * 1024 : nullptr;
        for (int i = threadIdx.x; i < 1024; i += kLaThreads) po[i] = pi ? pi[i] : 0.f;
    }
    if (idle) {
        if (a.gdst != a.gy) {
            const float4* s4 = reinterpret_cast<const float4*>(a.gy + so);
            float4* d4 = reinterpret_cast<float4*>(a.gdst + so);
            for (int q = jb0 * (kHop / 4) + threadIdx.x; q < jb1 * (kHop / 4); q += kLaThreads) d4[q] = s4[q];
        }
        if (a.dot && threadIdx.x == 0) {
            const size_t i = (size_t)b * a.pstride + blockIdx.x;
            a.pdot_out[i] = a.pdot_in[i];
        }
        return;
    }
    const ChainState cs = chain_state<false, ENV>(a, b, a.j0, a.upto, Ny, step, seed, dred, jb0 * kHop, gtab);

    const float4* y4 = reinterpret_cast<const float4*>(a.yraw + so);
    const float4* g4 = reinterpret_cast<const float4*>(a.gy + so);
    float4* gd4 = reinterpret_cast<float4*>(a.gdst + so);
    const float* gpL = (a.gpad && a.at_z) ? a.gpad + (size_t)b * 1024 : nullptr;
    const float* gpR = gpL ? gpL + 512 : nullptr;
    double dot = 0.0;
    for (int q = jb0 * (kHop / 4) + threadIdx.x; q < jb1 * (kHop / 4); q += kLaThreads) {
        const float4 yv = y4[q];
        const float4 gv = g4[q];
        float g[4] = {gv.x, gv.y, gv.z, gv.w};
        const float x[4] = {(yv.x * inv_m) * inv_m2, (yv.y * inv_m) * inv_m2, (yv.z * inv_m) * inv_m2, (yv.w * inv_m) * inv_m2};
        const int i0 = 4 * q;
        // reflect-pad parts of the streaming synthesis adjoint: pad[p] folds onto sample 512 - p, pad[u] of the right end
        // onto sample Ny - 2 - u (the staged adjoint has folded them already)
        if (gpL && (i0 <= kHalf || i0 + 3 >= Ny - kHalf - 1)) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = i0 + e;
                if (i >= 1 && i <= kHalf) g[e] += gpL[kHalf - i];
                if (i >= Ny - kHalf - 1 && i <= Ny - 2) g[e] += gpR[Ny - 2 - i];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if ((unsigned)(i0 + e) == cz.k) g[e] -= corr;
            g[e] = g[e] * inv_mm2;
        }
#pragma unroll
        for (int j = 0; j < kMaxLoopAttacks; ++j) {
            if (j >= a.j0 && j < a.upto && cs.on[j] && a.kind[j] == kLoopSampleSuppression) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if ((unsigned)(i0 + e - cs.start[j]) < (unsigned)a.k[j]) g[e] = 0.f;
            }
            if (ENV && j >= a.j0 && j < a.upto && cs.on[j] && a.kind[j] == kLoopGainEnvelope) {
                float ge[4];
                envelope_gain4(cs.env[j], gtab + j * kEnvTab, i0 - jb0 * kHop, ge);
#pragma unroll
                for (int e = 0; e < 4; ++e) g[e] = g[e] * ge[e];
            }
        }
        gd4[q] = make_float4(g[0], g[1], g[2], g[3]);
#pragma unroll
        for (int e = 0; e < 4; ++e) dot += (double)g[e] * (double)x[e];
    }
    if (!a.dot) return;
    dot = wave_sum_d(dot);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) dred[threadIdx.x >> 6] = dot;
    __syncthreads();
    if (threadIdx.x == 0) a.pdot_out[(size_t)b * a.pstride + blockIdx.x] = dred[0] + dred[1] + dred[2] + dred[3];
}

ChainArgs chain_args(const LoopAttackLaunch& L) {
    ChainArgs a{};
    a.frame_off = L.frame_off; a.pcount = L.pcount; a.pstride = L.pstride; a.run_blocks = L.run_blocks;
    a.step = L.step; a.step_back = L.step_back; a.seeds = L.seeds; a.n = L.n; a.j0 = 0; a.upto = L.n; a.B = L.B;
    a.src = L.yraw; a.norm = 1; a.at_z = 1; a.dot = 1; a.idle_plain = L.idle_plain; a.gpad_out = L.gpad_out;
    for (int j = 0; j < kMaxLoopAttacks; ++j) {
        a.kind[j] = j < L.n ? L.kind[j] : 0;
        a.k[j] = j < L.n ? L.k[j] : 0;
        a.inv_snr[j] = j < L.n ? L.inv_snr[j] : 0.0;
        a.prob[j] = j < L.n ? L.prob[j] : 0.f;
        a.p_lo[j] = j < L.n ? L.p_lo[j] : 0; a.p_hi[j] = j < L.n ? L.p_hi[j] : 0; a.floor[j] = j < L.n ? L.floor[j] : 0.f;
    }
    a.yraw = L.yraw; a.pmaxY = L.pmaxY; a.psq = L.psq; a.z = L.z; a.pmaxZ = L.pmaxZ;
    a.gate = L.gate;
    a.gy = L.gy; a.gdst = L.gy_out ? L.gy_out : L.gy; a.gpad = L.gpad; a.pdot_in = L.pdot_in; a.pdot_out = L.pdot_out;
    return a;
}

// whether entries [j0, j1) hold a gain envelope: the stage then launches the ENV instantiations
bool stage_has_envelope(const LoopAttackLaunch& L, int j0, int j1) {
    for (int j = j0; j < j1; ++j)
        if (L.kind[j] == kLoopGainEnvelope) return true;
    return false;
}

}  // namespace

void launch_loop_attack_stage(const LoopAttackLaunch& L, int j0, int j1, const float* src, int norm, float* dst,
                              unsigned long long* pmax, hipStream_t st) {
    ChainArgs a = chain_args(L);
    a.j0 = j0; a.src = src; a.norm = norm; a.z = dst; a.pmaxZ = pmax;
    const dim3 grid((unsigned)L.pstride, (unsigned)L.B, 1);
    // a noise entry's amplitude follows the power of the signal in front of it: one reduction per noise entry, in order
    for (int j = j0; j < j1; ++j) {
        if (L.kind[j] != kLoopGaussianNoise) continue;
        a.upto = j;
        if (stage_has_envelope(L, j0, j)) hipLaunchKernelGGL((chain_kernel<false, true>), grid, dim3(kLaThreads), 0, st, a);
        else hipLaunchKernelGGL((chain_kernel<false, false>), grid, dim3(kLaThreads), 0, st, a);
    }
    a.upto = j1;
    if (stage_has_envelope(L, j0, j1)) hipLaunchKernelGGL((chain_kernel<true, true>), grid, dim3(kLaThreads), 0, st, a);
    else hipLaunchKernelGGL((chain_kernel<true, false>), grid, dim3(kLaThreads), 0, st, a);
}

void launch_loop_attack_stage_bwd(const LoopAttackLaunch& L, int j0, int j1, int at_z, int dot, hipStream_t st) {
    ChainArgs a = chain_args(L);
    a.j0 = j0; a.upto = j1; a.at_z = at_z; a.dot = dot;
    const dim3 grid((unsigned)L.pstride, (unsigned)L.B, 1);
    if (stage_has_envelope(L, j0, j1)) hipLaunchKernelGGL(chain_bwd_kernel<true>, grid, dim3(kLaThreads), 0, st, a);
    else hipLaunchKernelGGL(chain_bwd_kernel<false>, grid, dim3(kLaThreads), 0, st, a);
}

void launch_loop_attack_forward(const LoopAttackLaunch& L, hipStream_t st) {
    launch_loop_attack_stage(L, 0, L.n, L.yraw, 1, L.z, L.pmaxZ, st);
}

void launch_loop_attack_backward(const LoopAttackLaunch& L, hipStream_t st) {
    launch_loop_attack_stage_bwd(L, 0, L.n, 1, 1, st);
}

}  // namespace aware
