// Attack-aware embedding on the general route (EXTENSION): the element-wise kinds of the loop's attack
// chains -- gaussian noise, sample suppression, gain envelope -- between the general loop's synthesis and its analysis, at any
// STFT geometry.  The model, the draws and the integer formulae are those of loop_attack_kernels.hip (its header comment
// states them); the torch restatement is aware_amd/embedding/loop_attacks.py::apply_chain.
//
//   x = N(N(yraw)),  z = chain(x),  a = N(N(z));  the loop's analysis reads a.        N(v) = v / (max|v| + 1e-8)
//
// What differs from the card's stage kernels is the layout.  A clip of the general route lies at out_off[b] = hop (frame_off[b]
// - b), Ny_b = hop (T_b - 1) samples long: any float offset, any length.  So the kernels work on a partition of their own, pieces
// of kGenChainPiece samples counted from the clip's first sample (one workgroup each, many per clip), and a thread's four
// samples 4 q .. 4 q + 3 of the clip are one Philox quad whatever the clip's address is: sample i uses the counter word it
// uses on the card route.  A quad goes through one float4 where the clip's offset is a multiple of four floats and the quad
// lies inside the clip, through guarded scalars otherwise.  Everything a clip needs as a whole travels as one partial per
// piece and is summed by every consumer workgroup in a fixed order, in f64 where the card kernels use f64, with no atomics:
// the same input gives the same bits from run to run, and from graph replay to eager launches.
//
//   gen_chain_kernel<false>   per noise entry: partial sums of x^2 in front of it
//   gen_chain_kernel<true>    z and the partial maxima of |z|
//   gen_chain_norm_kernel<false>  a = N(N(z)) from the partial maxima
//   gen_chain_norm_kernel<true>   partial sums of G * a, G = dL/da (the synthesis adjoint of the general route leaves none)
//   gen_chain_bwd_kernel      G -> dL/dx: the normalisers at z (scale 1 / (m m2), the arg-max sample also carries -sum * sign), the
//                             masks and the gains; partial sums of dL/dx * x
//   gen_chain_front_kernel    dL/dx -> dL/dyraw: the normalisers in front of the chain, in the same partial-sum form
// ENV instantiations hold the gain envelope; a chain without one launches kernels with none of its code or LDS.
#include "common.hpp"
#include "kernels.h"
#include "loop_any_chain.hpp"
#include "loop_gain.hpp"
#include "loop_stage.hpp"

namespace aware {

static_assert(kGenChainPiece <= kEnvSpan && kGenChainPiece % 4 == 0, "envelope_block's table; one Philox quad per thread");

namespace {

constexpr int kGcThreads = 256;
constexpr int kGcQuads = kGenChainPiece / 4;      // quads per piece

struct GenChainArgs {
    const int* sig_off; const int* sig_len; const int* pc_out;
    int B, pstride, pieces;
    const int* step; int step_back;
    const unsigned* seeds;
    int n, upto;                          // entries [0, upto) are applied (sums of squares: those in front of noise entry `upto`)
    int kind[kMaxLoopAttacks];
    int k[kMaxLoopAttacks];
    double inv_snr[kMaxLoopAttacks];
    float prob[kMaxLoopAttacks];
    int p_lo[kMaxLoopAttacks], p_hi[kMaxLoopAttacks];
    float floor[kMaxLoopAttacks];
    const float* yraw; const unsigned long long* pmaxY;
    double* psq; float* z; unsigned long long* pmaxZ; float* a;
    float* gy; double* pdotA; double* pdotX;
};

// one workgroup's piece of clip b
struct Piece {
    int so, n;          // the clip: n floats at offset so
    int np;             // its pieces
    int q0, q1;         // this piece's quads [q0, q1) of the clip
    bool vec;           // the clip's quads are 16-byte aligned
};
// false where the clip has no such piece; uniform over the workgroup
__device__ __forceinline__ bool piece_enter(const GenChainArgs& a, int b, Piece& p) {
    p.so = a.sig_off[b]; p.n = a.sig_len[b];
    p.np = max(1, (p.n + kGenChainPiece - 1) / kGenChainPiece);
    if ((int)blockIdx.x >= p.np) return false;
    p.q0 = blockIdx.x * kGcQuads;
    p.q1 = min(p.q0 + kGcQuads, (p.n + 3) >> 2);
    p.vec = (p.so & 3) == 0;
    return true;
}
// v = s[i .. i + 3] of a clip of n samples (zero from n on); every signal array is 256-byte aligned at its first clip
__device__ __forceinline__ void load_quad(const float* s, const Piece& p, int i, float (&v)[4]) {
    if (p.vec && i + 3 < p.n) {
        const float4 t = *reinterpret_cast<const float4*>(s + i);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = i + e < p.n ? s[i + e] : 0.f;
    }
}
__device__ __forceinline__ void store_quad(float* s, const Piece& p, int i, const float (&v)[4]) {
    if (p.vec && i + 3 < p.n) {
        *reinterpret_cast<float4*>(s + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i + e < p.n) s[i + e] = v[e];
    }
}

// sum of a clip's f64 partials in a fixed order; all threads of the block call this
__device__ __forceinline__ double block_sum_d(const double* part, int n, double* dred) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kGcThreads) s += part[i];
    s = wave_sum_d(s);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) dred[threadIdx.x >> 6] = s;
    __syncthreads();
    return dred[0] + dred[1] + dred[2] + dred[3];
}
// the workgroup's own partial sum into part[0]
__device__ __forceinline__ void block_store_d(double v, double* part, double* dred) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) dred[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) *part = dred[0] + dred[1] + dred[2] + dred[3];
}

// per-clip state of the chain at this step, as chain_state of loop_attack_kernels.hip computes it: which entries fire, where
// the suppressions start, the noise amplitudes, the envelopes' geometry on this piece
struct GcState {
    bool on[kMaxLoopAttacks];
    int start[kMaxLoopAttacks];
    float sigma[kMaxLoopAttacks];
    EnvBlock env[kMaxLoopAttacks];
};
template <bool SIGMA, bool ENV>
__device__ __forceinline__ GcState chain_state(const GenChainArgs& a, int b, const Piece& p, unsigned step, unsigned seed,
                                               double* dred, float* gtab) {
    GcState cs;
#pragma unroll
    for (int j = 0; j < kMaxLoopAttacks; ++j) {
        cs.on[j] = false; cs.start[j] = 0; cs.sigma[j] = 0.f;
        if (ENV) cs.env[j] = EnvBlock{kEnvelopeMinPeriod, 0.f, 0, 0};
        if (j < a.upto) {
            unsigned r[4];
            philox4x32_10(0u, step, 1u + (unsigned)j, 1u, seed, 0x5EEDu, r);
            cs.on[j] = loop_entry_fires(r[0], a.prob[j]);
            if (a.kind[j] == kLoopSampleSuppression) {
                cs.start[j] = loop_below(r[1], p.n - a.k[j]);
            } else if (a.kind[j] == kLoopGainEnvelope) {
                if (ENV && cs.on[j]) {
                    int P, ph;
                    envelope_draw(r, a.p_lo[j], a.p_hi[j], P, ph);
                    cs.env[j] = envelope_block(gtab + j * kEnvTab, 4 * p.q0, P, ph, a.floor[j], step, (unsigned)j, seed);
                }
            } else if (SIGMA) {
                const double ss = block_sum_d(a.psq + ((size_t)j * a.B + b) * a.pieces, p.np, dred);
                cs.sigma[j] = (float)sqrt(ss / (double)p.n * a.inv_snr[j]);
            }
        }
    }
    if (ENV) __syncthreads();             // the tables are complete
    return cs;
}
// the masks and the gains of entries [0, upto) on the quad at sample i0: what the forward and the backward pass share
template <bool ENV>
__device__ __forceinline__ void mask_gain(const GenChainArgs& a, const GcState& cs, const float* gtab, int j, int i0, int i_first,
                                          float (&v)[4]) {
    if (a.kind[j] == kLoopSampleSuppression) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if ((unsigned)(i0 + e - cs.start[j]) < (unsigned)a.k[j]) v[e] = 0.f;
    } else if (ENV && a.kind[j] == kLoopGainEnvelope) {
        float g[4];
        envelope_gain4(cs.env[j], gtab + j * kEnvTab, i0 - i_first, g);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] * g[e];
    }
}

// WRITE = false: partial sums of x^2 with the entries in front of `upto` applied; true: the whole chain, z and max|z|
template <bool WRITE, bool ENV>
__global__ __launch_bounds__(kGcThreads) void gen_chain_kernel(GenChainArgs a) {
    __shared__ unsigned long long red[4];
    __shared__ double dred[4];
    __shared__ float gtab[ENV ? kMaxLoopAttacks * kEnvTab : 1];
    const int b = blockIdx.y;
    Piece p;
    if (!piece_enter(a, b, p)) return;
    const ClipNorm cn = clip_norm_from_partials(a.pmaxY + (size_t)b * a.pstride, a.pc_out[b], red);
    const float inv_m = 1.0f / cn.m, inv_m2 = 1.0f / cn.m2;
    const unsigned step = (unsigned)(*a.step - a.step_back), seed = a.seeds[b];
    const GcState cs = chain_state<true, ENV>(a, b, p, step, seed, dred, gtab);

    const float* y = a.yraw + p.so;
    float* z = a.z + p.so;
    unsigned long long best = 0;
    double acc = 0.0;
    for (int q = p.q0 + threadIdx.x; q < p.q1; q += kGcThreads) {
        const int i0 = 4 * q;
        float v[4];
        load_quad(y, p, i0, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (v[e] * inv_m) * inv_m2;
#pragma unroll
        for (int j = 0; j < kMaxLoopAttacks; ++j) {
            if (j < a.upto && cs.on[j]) {
                if (a.kind[j] == kLoopGaussianNoise) {
                    float eps[4];
                    normal4((unsigned)q, step, (unsigned)j, seed, eps);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = v[e] + cs.sigma[j] * eps[e];
                } else {
                    mask_gain<ENV>(a, cs, gtab, j, i0, 4 * p.q0, v);
                }
            }
        }
        if (WRITE) {
            store_quad(z, p, i0, v);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i0 + e < p.n) best = umax64(best, pack_max(fabsf(v[e]), (unsigned)(i0 + e)));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i0 + e < p.n) acc += (double)v[e] * (double)v[e];
        }
    }
    if (WRITE) {
        best = wave_max64(best);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
        __syncthreads();
        if (threadIdx.x == 0)
            a.pmaxZ[(size_t)b * a.pieces + blockIdx.x] = umax64(umax64(red[0], red[1]), umax64(red[2], red[3]));
    } else {
        block_store_d(acc, a.psq + ((size_t)a.upto * a.B + b) * a.pieces + blockIdx.x, dred);
    }
}

// a = N(N(z)); DOT: instead, the partial sums of gy * a
template <bool DOT>
__global__ __launch_bounds__(kGcThreads) void gen_chain_norm_kernel(GenChainArgs a) {
    __shared__ unsigned long long red[4];
    __shared__ double dred[4];
    const int b = blockIdx.y;
    Piece p;
    if (!piece_enter(a, b, p)) return;
    float inv_m = 1.0f, inv_m2 = 1.0f;
    if (!DOT) {
        const ClipNorm cz = clip_norm_from_partials(a.pmaxZ + (size_t)b * a.pieces, p.np, red);
        inv_m = 1.0f / cz.m; inv_m2 = 1.0f / cz.m2;
    }
    double dot = 0.0;
    for (int q = p.q0 + threadIdx.x; q < p.q1; q += kGcThreads) {
        float v[4];
        if (DOT) {
            float g[4];
            load_quad(a.a + p.so, p, 4 * q, v);
            load_quad(a.gy + p.so, p, 4 * q, g);
#pragma unroll
            for (int e = 0; e < 4; ++e) dot += (double)g[e] * (double)v[e];      // both zero from n on
        } else {
            load_quad(a.z + p.so, p, 4 * q, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (v[e] * inv_m) * inv_m2;
            store_quad(a.a + p.so, p, 4 * q, v);
        }
    }
    if (DOT) block_store_d(dot, a.pdotA + (size_t)b * a.pieces + blockIdx.x, dred);
}

// gy holds G = dL/da, pdotA the partial sums of G * a.  Backward of the two normalisers at z, identity through the noise (sigma
// is a constant), the 0 / 1 masks, the gains (all diagonal: their order is free).  The result replaces G; its partial sums
// against x = N(N(yraw)) go to pdotX
template <bool ENV>
__global__ __launch_bounds__(kGcThreads) void gen_chain_bwd_kernel(GenChainArgs a) {
    __shared__ unsigned long long red[4];
    __shared__ double dred[4];
    __shared__ float gtab[ENV ? kMaxLoopAttacks * kEnvTab : 1];
    const int b = blockIdx.y;
    Piece p;
    if (!piece_enter(a, b, p)) return;
    const ClipNorm cy = clip_norm_from_partials(a.pmaxY + (size_t)b * a.pstride, a.pc_out[b], red);
    const ClipNorm cz = clip_norm_from_partials(a.pmaxZ + (size_t)b * a.pieces, p.np, red);
    const float inv_m = 1.0f / cy.m, inv_m2 = 1.0f / cy.m2;
    const float inv_mm2 = 1.0f / (cz.m * cz.m2);
    const float adot = (float)block_sum_d(a.pdotA + (size_t)b * a.pieces, p.np, dred);
    const unsigned kz = min(cz.k, (unsigned)(p.n - 1));
    const float zk = a.z[p.so + kz];
    const float corr = adot * ((zk > 0.f) ? 1.f : ((zk < 0.f) ? -1.f : 0.f));
    const unsigned step = (unsigned)(*a.step - a.step_back), seed = a.seeds[b];
    const GcState cs = chain_state<false, ENV>(a, b, p, step, seed, dred, gtab);

    float* gy = a.gy + p.so;
    double dot = 0.0;
    for (int q = p.q0 + threadIdx.x; q < p.q1; q += kGcThreads) {
        const int i0 = 4 * q;
        float x[4], g[4];
        load_quad(a.yraw + p.so, p, i0, x);
        load_quad(gy, p, i0, g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            x[e] = (x[e] * inv_m) * inv_m2;
            if ((unsigned)(i0 + e) == kz) g[e] -= corr;
            g[e] = g[e] * inv_mm2;
        }
#pragma unroll
        for (int j = 0; j < kMaxLoopAttacks; ++j)
            if (j < a.upto && cs.on[j]) mask_gain<ENV>(a, cs, gtab, j, i0, 4 * p.q0, g);
        store_quad(gy, p, i0, g);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i0 + e < p.n) dot += (double)g[e] * (double)x[e];
    }
    block_store_d(dot, a.pdotX + (size_t)b * a.pieces + blockIdx.x, dred);
}

// gy holds dL/dx, pdotX the partial sums of dL/dx * x: backward of the two normalisers in front of the chain, in place
__global__ __launch_bounds__(kGcThreads) void gen_chain_front_kernel(GenChainArgs a) {
    __shared__ unsigned long long red[4];
    __shared__ double dred[4];
    const int b = blockIdx.y;
    Piece p;
    if (!piece_enter(a, b, p)) return;
    const ClipNorm cy = clip_norm_from_partials(a.pmaxY + (size_t)b * a.pstride, a.pc_out[b], red);
    const float inv_mm2 = 1.0f / (cy.m * cy.m2);
    const float xdot = (float)block_sum_d(a.pdotX + (size_t)b * a.pieces, p.np, dred);
    const unsigned ky = min(cy.k, (unsigned)(p.n - 1));
    const float yk = a.yraw[p.so + ky];
    const float corr = xdot * ((yk > 0.f) ? 1.f : ((yk < 0.f) ? -1.f : 0.f));
    float* gy = a.gy + p.so;
    for (int q = p.q0 + threadIdx.x; q < p.q1; q += kGcThreads) {
        const int i0 = 4 * q;
        float g[4];
        load_quad(gy, p, i0, g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if ((unsigned)(i0 + e) == ky) g[e] -= corr;
            g[e] = g[e] * inv_mm2;
        }
        store_quad(gy, p, i0, g);
    }
}

GenChainArgs gen_chain_args(const GenChainLaunch& L) {
    GenChainArgs a{};
    a.sig_off = L.sig_off; a.sig_len = L.sig_len; a.pc_out = L.pc_out; a.B = L.B; a.pstride = L.pstride; a.pieces = L.pieces;
    a.step = L.step; a.step_back = L.step_back; a.seeds = L.seeds; a.n = L.n; a.upto = L.n;
    for (int j = 0; j < kMaxLoopAttacks; ++j) {
        const bool in = j < L.n;
        a.kind[j] = in ? L.kind[j] : 0; a.k[j] = in ? L.k[j] : 0; a.inv_snr[j] = in ? L.inv_snr[j] : 0.0;
        a.prob[j] = in ? L.prob[j] : 0.f; a.p_lo[j] = in ? L.p_lo[j] : 0; a.p_hi[j] = in ? L.p_hi[j] : 0;
        a.floor[j] = in ? L.floor[j] : 0.f;
    }
    a.yraw = L.yraw; a.pmaxY = L.pmaxY; a.psq = L.psq; a.z = L.z; a.pmaxZ = L.pmaxZ; a.a = L.a;
    a.gy = L.gy; a.pdotA = L.pdotA; a.pdotX = L.pdotX;
    return a;
}
// whether entries [0, upto) hold a gain envelope: the launch then takes the ENV instantiation
bool has_envelope(const GenChainLaunch& L, int upto) {
    for (int j = 0; j < upto; ++j)
        if (L.kind[j] == kLoopGainEnvelope) return true;
    return false;
}

}  // namespace

void launch_gen_chain_forward(const GenChainLaunch& L, hipStream_t st) {
    GenChainArgs a = gen_chain_args(L);
    const dim3 grid((unsigned)L.pieces, (unsigned)L.B, 1), blk(kGcThreads);
    // a noise entry's amplitude follows the power of the signal in front of it: one reduction per noise entry, in order
    for (int j = 0; j < L.n; ++j) {
        if (L.kind[j] != kLoopGaussianNoise) continue;
        a.upto = j;
        if (has_envelope(L, j)) hipLaunchKernelGGL((gen_chain_kernel<false, true>), grid, blk, 0, st, a);
        else hipLaunchKernelGGL((gen_chain_kernel<false, false>), grid, blk, 0, st, a);
    }
    a.upto = L.n;
    if (has_envelope(L, L.n)) hipLaunchKernelGGL((gen_chain_kernel<true, true>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((gen_chain_kernel<true, false>), grid, blk, 0, st, a);
    hipLaunchKernelGGL(gen_chain_norm_kernel<false>, grid, blk, 0, st, a);
}

void launch_gen_chain_backward(const GenChainLaunch& L, hipStream_t st) {
    const GenChainArgs a = gen_chain_args(L);
    const dim3 grid((unsigned)L.pieces, (unsigned)L.B, 1), blk(kGcThreads);
    hipLaunchKernelGGL(gen_chain_norm_kernel<true>, grid, blk, 0, st, a);
    if (has_envelope(L, L.n)) hipLaunchKernelGGL(gen_chain_bwd_kernel<true>, grid, blk, 0, st, a);
    else hipLaunchKernelGGL(gen_chain_bwd_kernel<false>, grid, blk, 0, st, a);
    hipLaunchKernelGGL(gen_chain_front_kernel, grid, blk, 0, st, a);
}

}  // namespace aware
