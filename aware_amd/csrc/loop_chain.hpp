// The host-only logic of the embed loop's attack chains (aware_embed_set_loop_attacks[_ex], aware_embed_set_loop_mixture): one
// chain's state, the parser with every AWARE_E_BADARG / AWARE_E_UNSUPPORTED of the setters, and the carving of the chains'
// workspace.  Plain C++: no HIP header and no HIP call, so tests/host_sim/loop_chain_check.cpp runs it on the CPU.
//
// THE ONE-SPLIT RULE.  loop_kind_staged (loop_limits.hpp: kLoopKindTable's splitting rows and the kinds of kLoopStagedBeyond) says
// of every kind whether it is element-wise and runs inside the stage kernels of loop_attack_kernels.hip, or needs launches of
// its own between two such stages: it SPLITS the chain.  A chain holds at
// most one splitting entry.  The one exception: a speed change directly behind a time stretch (j == split + 1) forms one stage
// u -> v -> z with it.  The host twin is embedding/loop_attacks.py::parse_chain (TABLE, SPLITTING, STAGED).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "../../include/aware_hip.h"
#include "loop_limits.hpp"

namespace aware {

// complex f32 of the chains' spectra: the kernels' cf where a HIP translation unit defines AWARE_LOOP_CF before including
// this header, a plain pair of the same size otherwise
#ifndef AWARE_LOOP_CF
struct LoopCf { float re, im; };
#define AWARE_LOOP_CF LoopCf
#endif

// workspace carving: pointer arithmetic only
struct Carver {
    char* base;       // null: only count (off is then the workspace size)
    size_t off = 0, cap;
    bool ok = true;
    Carver(void* p, size_t c) : base((char*)p), cap(c) {}
    template <typename Tp> Tp* take(size_t count) {
        off = (off + 255) & ~(size_t)255;
        Tp* r = base ? (Tp*)(base + off) : nullptr;
        off += count * sizeof(Tp);
        if (off > cap) ok = false;
        return r;
    }
};

// what the parser and the carver read of a batch
struct LoopDims {
    int B = 0, NS = 0, NF = 0, pstride = 0;
    const int* out_len = nullptr;                 // [B]
};

// one chain and its buffers in the caller's second workspace.  n == 0: the loop issues exactly the launches of the plain loop
struct LoopChainState {
    using cf = AWARE_LOOP_CF;
    int n = 0;
    int kind[kMaxLoopAttacks] = {0}, k[kMaxLoopAttacks] = {0};
    double inv_snr[kMaxLoopAttacks] = {0};
    float prob[kMaxLoopAttacks] = {0};
    int p_lo[kMaxLoopAttacks] = {0}, p_hi[kMaxLoopAttacks] = {0};      // gain envelope: samples between breakpoints, drawn in [p_lo, p_hi]
    float floor[kMaxLoopAttacks] = {0};       // gain envelope: the lowest gain
    float* z = nullptr;                       // [NS] the attacked signal
    unsigned long long* pmaxZ = nullptr;      // [B][pstride]
    double* psq = nullptr;                    // [kMaxLoopAttacks][B][pstride] partial sums of squares per noise entry
    double* pdot = nullptr;                   // [B][pstride] partial sums of dL/dx * x for the analysis adjoint
    float* gpad0 = nullptr;                   // [B][2][512] zeros: the pads are folded before the analysis adjoint
    unsigned* seeds = nullptr;                // [B]
    // the splitting entry (the rule is at the top of this file): its index, -1 without one, and its kind.  pair_speed: the
    // speed change directly behind a time stretch (split + 1), -1 without one.  What each kind reads of the parameters:
    //   reverberation   lo..hi: taps of the impulse response; gain: 10^(drr_db / 20); kmax: blocks of the longest clip
    //   speed change    lo..hi: speed offsets
    //   time stretch    lo..hi: stretch offsets; lo2..hi2: the speed offsets of pair_speed
    //   pitch shift     lo..hi: speed offsets
    //   phase vocoder   lo..hi: stretch offsets, lo2..hi2: speed offsets; lo > hi where the mode is absent
    //   sample deletion lo..hi: samples cut out; at 0: the cut starts at sample 0, 1: anywhere
    //   band filter     lo..hi: edges in 1 / 65536 cycle per sample; mask: the responses drawn from; w_min: a band's least width
    //   tiled excerpt   lo..hi: samples of the excerpt
    //   time warp       lo..hi: exponents e of the 2^e samples between breakpoints; depth: the widest rate offset D; kmax:
    //                   breakpoints of the longest clip at 2^lo
    //   frequency shift lo..hi: shifts d in units of sr / 2^20 Hz, signed
    int split = -1, split_kind = 0, pair_speed = -1;
    int lo = 0, hi = 0, lo2 = 0, hi2 = -1, at = 0, kmax = 0, mask = 0, w_min = 0, depth = 0;
    double gain = 0;
    float* u = nullptr;                       // [NS] the splitting stage's input: the entries in front of it on N(N(yraw))
    float* h = nullptr;                       // [B][8192] the impulse responses of the last forward pass
    int* nh = nullptr;                        // [B] their lengths, 0 where the entry did not fire
    cf* tables = nullptr;                     // W_2048 half table, W_4096 table
    cf* hspec = nullptr;                      // [B][4][2056]
    cf* xspec = nullptr;                      // [B][kmax][2056]
    float* v = nullptr;                       // [NS] between the stretch and the speed change of a pair
    cf* pvS = nullptr;                        // [NF][520] the spectrum of u; the backward pass turns it into its gradient
    cf* pvY = nullptr;                        // [NF][520] the vocoded spectrum; the backward pass holds dL/dY in it
    int* warpR = nullptr;                     // [B][kmax] the rates R_k = 65536 + m_k of the last forward pass's time warp
    long long* warpA = nullptr;               // [B][kmax] the positions A(k) at its breakpoints, 16.16 fixed point
    const float* hann = nullptr;              // stretch_window()
    bool locked = false;                      // an optimiser step has run: the chain stays what it is
    LoopGate gate;                            // a chain of a mixture: the clips that drew it (null: every clip)
};

inline bool chain_splits(const LoopChainState& la) { return la.split >= 0; }
inline bool chain_has(const LoopChainState& la, int kind) { return chain_splits(la) && la.split_kind == kind; }

// lo <= hi, both integers inside [min, max]
inline bool int_range(float lo, float hi, float min, float max) {
    return lo >= min && hi <= max && lo <= hi && lo == floorf(lo) && hi == floorf(hi);
}

// one chain's entries into its state: every AWARE_E_BADARG / AWARE_E_UNSUPPORTED of the setters, no buffer touched.
// ex: the entry points with four parameters per entry; the older pair refuses the splitting kinds
inline int parse_loop_chain(const LoopDims& d, const aware_loop_attack_ex* attacks, int n_attacks, bool ex, LoopChainState& la) {
    static_assert(AWARE_LOOP_GAUSSIAN_NOISE == kLoopGaussianNoise && AWARE_LOOP_SAMPLE_SUPPRESSION == kLoopSampleSuppression &&
                  AWARE_LOOP_REVERBERATION == kLoopReverberation && AWARE_LOOP_SPEED_CHANGE == kLoopSpeedChange &&
                  AWARE_LOOP_TIME_STRETCH == kLoopTimeStretch && AWARE_LOOP_PITCH_SHIFT == kLoopPitchShift &&
                  AWARE_LOOP_PHASE_VOCODER == kLoopPhaseVocoder && AWARE_LOOP_DELETE_SAMPLES == kLoopDeleteSamples &&
                  AWARE_LOOP_GAIN_ENVELOPE == kLoopGainEnvelope && AWARE_LOOP_BAND_FILTER == kLoopBandFilter &&
                  AWARE_LOOP_EXCERPT == kLoopExcerpt && AWARE_LOOP_TIME_WARP == kLoopTimeWarp &&
                  AWARE_LOOP_FREQUENCY_SHIFT == kLoopFrequencyShift, "");
    if (!attacks || n_attacks < 1 || n_attacks > kMaxLoopAttacks) return AWARE_E_BADARG;
    la.split = -1; la.pair_speed = -1; la.h = nullptr; la.v = nullptr;
    for (int j = 0; j < n_attacks; ++j) {
        const aware_loop_attack_ex& a = attacks[j];
        const float* p = a.param;
        if (!(a.prob >= 0.f && a.prob <= 1.f)) return AWARE_E_BADARG;
        la.kind[j] = a.kind; la.prob[j] = a.prob; la.k[j] = 0; la.inv_snr[j] = 0.0;
        la.p_lo[j] = 0; la.p_hi[j] = 0; la.floor[j] = 0.f;
        if (a.kind < 0 || a.kind >= kLoopKinds || (kLoopKindTable[a.kind].ex_only && !ex)) return AWARE_E_BADARG;
        const bool splits = loop_kind_staged(a.kind);
        // the one-split rule
        const bool pair = chain_has(la, AWARE_LOOP_TIME_STRETCH) && a.kind == AWARE_LOOP_SPEED_CHANGE && j == la.split + 1;
        if (splits && chain_splits(la) && !pair) return AWARE_E_BADARG;
        switch (a.kind) {            // the parameters' validation; a splitting kind's range is integers in range behind it
            case AWARE_LOOP_GAUSSIAN_NOISE:
                if (!std::isfinite(p[0])) return AWARE_E_BADARG;
                la.inv_snr[j] = pow(10.0, -(double)p[0] / 10.0);
                break;
            case AWARE_LOOP_SAMPLE_SUPPRESSION:
                if (!(p[0] >= 1.f) || p[0] > 2147483520.f || p[0] != floorf(p[0])) return AWARE_E_BADARG;
                la.k[j] = (int)p[0];
                break;
            case AWARE_LOOP_GAIN_ENVELOPE:      // param = {P_lo, P_hi, floor, 0}
                if (!int_range(p[0], p[1], (float)kEnvelopeMinPeriod, (float)kEnvelopeMaxPeriod) || !(p[2] >= 0.f && p[2] < 1.f))
                    return AWARE_E_BADARG;
                la.p_lo[j] = (int)p[0]; la.p_hi[j] = (int)p[1]; la.floor[j] = p[2];
                break;
            case AWARE_LOOP_REVERBERATION:
                if (!int_range(p[0], p[1], 2.f, (float)kReverbMaxIr) || !std::isfinite(p[2])) return AWARE_E_BADARG;
                la.gain = pow(10.0, (double)p[2] / 20.0);
                break;
            case AWARE_LOOP_SPEED_CHANGE:
            case AWARE_LOOP_PITCH_SHIFT:
                if (!int_range(p[0], p[1], (float)kSpeedMin, (float)kSpeedMax)) return AWARE_E_BADARG;
                break;
            case AWARE_LOOP_TIME_STRETCH:
                if (!int_range(p[0], p[1], (float)kStretchMin, (float)kStretchMax)) return AWARE_E_BADARG;
                break;
            case AWARE_LOOP_PHASE_VOCODER: {
                // param = {mq_lo, mq_hi, m_lo, m_hi}: a mode with lo > hi is absent, and one of the two is there
                for (int i = 0; i < 4; ++i)
                    if (!(fabsf(p[i]) <= 65536.f) || p[i] != floorf(p[i])) return AWARE_E_BADARG;
                const int ql = (int)p[0], qh = (int)p[1], ml = (int)p[2], mh = (int)p[3];
                if (ql > qh && ml > mh) return AWARE_E_BADARG;
                if (ql <= qh && (ql < kStretchMin || qh > kStretchMax)) return AWARE_E_BADARG;
                if (ml <= mh && (ml < kSpeedMin || mh > kSpeedMax)) return AWARE_E_BADARG;
                la.lo2 = ml; la.hi2 = mh;
                break;
            }
            case AWARE_LOOP_BAND_FILTER:      // param = {mask, c_lo, c_hi, w_min}
                if (!int_range(p[0], p[0], 1.f, 15.f) || !int_range(p[1], p[2], 1.f, (float)kFilterMaxEdge) ||
                    !int_range(p[3], p[3], 1.f, (float)kFilterMaxEdge) || p[2] + p[3] > (float)kFilterMaxEdge)
                    return AWARE_E_BADARG;
                la.mask = (int)p[0]; la.w_min = (int)p[3];
                break;
            case AWARE_LOOP_EXCERPT:          // param = {L_lo, L_hi, 0, 0}; a clip shorter than L_lo is left alone, not refused
                if (!int_range(p[0], p[1], (float)kExcerptMinLen, 2147483520.f) || p[2] != 0.f || p[3] != 0.f) return AWARE_E_BADARG;
                break;
            case AWARE_LOOP_TIME_WARP:        // param = {e_lo, e_hi, D, 0}; D >= 1: a warp of depth 0 is no entry
                if (!int_range(p[0], p[1], (float)kWarpMinExp, (float)kWarpMaxExp) || !int_range(p[2], p[2], 1.f, (float)kWarpMaxDepth) ||
                    p[3] != 0.f)
                    return AWARE_E_BADARG;
                la.depth = (int)p[2];
                break;
            case AWARE_LOOP_FREQUENCY_SHIFT:  // param = {d_lo, d_hi, 0, 0}, in units of sr / 2^20 Hz, signed
                if (!int_range(p[0], p[1], -(float)kShiftMax, (float)kShiftMax) || p[2] != 0.f || p[3] != 0.f) return AWARE_E_BADARG;
                break;
            default:    // AWARE_LOOP_DELETE_SAMPLES, param = {k_lo, k_hi, at, 0}
                if (!int_range(p[0], p[1], 1.f, 2147483520.f) || !(p[2] == 0.f || p[2] == 1.f)) return AWARE_E_BADARG;
                la.at = (int)p[2];
                break;
        }
        if (!splits) continue;
        if (pair) { la.pair_speed = j; la.lo2 = (int)p[0]; la.hi2 = (int)p[1]; }
        else {
            const int first = a.kind == AWARE_LOOP_BAND_FILTER ? 1 : 0;      // the band filter's range follows its mask
            la.split = j; la.split_kind = a.kind; la.lo = (int)p[first]; la.hi = (int)p[first + 1];
        }
    }
    for (int j = 0; j < n_attacks; ++j)
        for (int i = 0; i < d.B; ++i)
            if ((la.kind[j] == AWARE_LOOP_SAMPLE_SUPPRESSION && la.k[j] >= d.out_len[i]) ||
                (la.kind[j] == AWARE_LOOP_DELETE_SAMPLES && la.hi >= d.out_len[i]))
                return AWARE_E_UNSUPPORTED;
    la.n = n_attacks;
    return AWARE_OK;
}

// A chain that the parser refuses with AWARE_E_BADARG still has the byte count aware_embed_loop_attack_workspace_bytes_ex
// has always answered for it: that of the first of its splitting entries of the lowest refused_rank (kLoopKindTable), with a
// pair's v if a time stretch decides and a speed change stands anywhere
inline void size_refused_chain(const aware_loop_attack_ex* attacks, int n_attacks, LoopChainState& la) {
    la.split = -1; la.pair_speed = -1;
    for (int j = 0; j < n_attacks; ++j) {
        const int kind = attacks[j].kind;
        if (kind < 0 || kind >= kLoopKinds || !loop_kind_staged(kind)) continue;
        if (!chain_splits(la) || loop_staged_rank(kind) < loop_staged_rank(la.split_kind)) {
            la.split = j; la.split_kind = kind;
        }
    }
    for (int j = 0; j < n_attacks && chain_has(la, AWARE_LOOP_TIME_STRETCH); ++j)
        if (attacks[j].kind == AWARE_LOOP_SPEED_CHANGE) la.pair_speed = j;
}

// The chains' buffers live in a workspace of their own, so that aware_embed_workspace_bytes and the layout of the loop's
// workspace stay what they were.  What every chain needs (a mixture's chains share it):
inline void carve_chain_shared(Carver& c, const LoopDims& d, LoopChainState& la) {
    const size_t np = (size_t)d.B * d.pstride;
    la.z = c.take<float>(d.NS);
    la.pmaxZ = c.take<unsigned long long>(np);
    la.psq = c.take<double>(np * kMaxLoopAttacks);
    la.pdot = c.take<double>(np);
    la.gpad0 = c.take<float>((size_t)d.B * 1024);
    la.seeds = c.take<unsigned>(d.B);
}
// ... and what a chain's backward pass needs from its forward pass
inline void carve_chain_private(Carver& c, const LoopDims& d, LoopChainState& la) {
    using cf = LoopChainState::cf;
    if (chain_has(la, AWARE_LOOP_REVERBERATION)) {
        la.kmax = reverb_blocks(*std::max_element(d.out_len, d.out_len + d.B));
        la.h = c.take<float>((size_t)d.B * kReverbMaxIr);
        la.nh = c.take<int>(d.B);
        la.tables = c.take<cf>(kReverbTwHalf + kReverbBins);
        la.hspec = c.take<cf>((size_t)d.B * kReverbParts * kReverbBins);
        la.xspec = c.take<cf>((size_t)d.B * la.kmax * kReverbBins);
    } else if (chain_has(la, AWARE_LOOP_PHASE_VOCODER)) {
        la.pvS = c.take<cf>((size_t)d.NF * 520);
        la.pvY = c.take<cf>((size_t)d.NF * 520);
    } else if (chain_has(la, AWARE_LOOP_TIME_WARP)) {
        // a refused chain is sized too (size_refused_chain): its exponent may be unset
        const int e_lo = std::min(std::max(la.lo, kWarpMinExp), kWarpMaxExp);
        la.kmax = warp_breakpoints(*std::max_element(d.out_len, d.out_len + d.B), e_lo);
        la.warpR = c.take<int>((size_t)d.B * la.kmax);
        la.warpA = c.take<long long>((size_t)d.B * la.kmax);
    } else if (la.pair_speed >= 0) {
        la.v = c.take<float>(d.NS);
    }
}
// a plain handle: the shared part, the one signal u a splitting entry reads, the private part
inline void carve_loop_chain(Carver& c, const LoopDims& d, LoopChainState& la) {
    carve_chain_shared(c, d, la);
    if (chain_splits(la)) la.u = c.take<float>(d.NS);
    carve_chain_private(c, d, la);
}
// A mixture: what the chains share (u if one of them splits), then per chain its private part, then the choices.  For one
// chain this is the layout of aware_embed_set_loop_attacks_ex followed by int [B] at the next 256-byte boundary.
inline void carve_loop_mixture(Carver& c, const LoopDims& d, LoopChainState& shared, LoopChainState* mix, int n, int*& choice) {
    carve_chain_shared(c, d, shared);
    const bool any_u = std::any_of(mix, mix + n, chain_splits);
    shared.u = any_u ? c.take<float>(d.NS) : nullptr;
    for (int i = 0; i < n; ++i) {
        LoopChainState& la = mix[i];
        la.z = shared.z; la.pmaxZ = shared.pmaxZ; la.psq = shared.psq; la.pdot = shared.pdot; la.gpad0 = shared.gpad0;
        la.seeds = shared.seeds; la.u = shared.u;
        carve_chain_private(c, d, la);
    }
    choice = c.take<int>(d.B);
}

// T_c = min(floor((w_0 + .. + w_c) 2^32), 2^32) from the float32 weights, summed in double
inline void loop_mix_thresholds(const float* weights, int n, unsigned long long* thr) {
    double acc = 0.0;
    for (int c = 0; c < kMaxLoopChains; ++c) {
        if (c < n) acc += (double)weights[c];
        const double t = std::floor(acc * 4294967296.0);
        thr[c] = c < n ? (t >= 4294967296.0 ? 4294967296ull : (t > 0.0 ? (unsigned long long)t : 0ull)) : 0ull;
    }
}
// the chains and weights into states and thresholds; rc as the setter's.  mix_rv: the chain with the reverberation
inline int parse_loop_mixture(const LoopDims& d, const aware_loop_chain* chains, int n_chains, LoopChainState* mix,
                              unsigned long long* thr, int& mix_rv) {
    if (!chains || n_chains < 1 || n_chains > kMaxLoopChains) return AWARE_E_BADARG;
    float w[kMaxLoopChains] = {0};
    double sum = 0.0;
    mix_rv = -1;
    for (int i = 0; i < n_chains; ++i) {
        if (!std::isfinite(chains[i].weight) || chains[i].weight < 0.f) return AWARE_E_BADARG;
        w[i] = chains[i].weight; sum += (double)w[i];
        mix[i] = LoopChainState();
        if (int rc = parse_loop_chain(d, chains[i].attacks, chains[i].n_attacks, true, mix[i])) return rc;
        if (chain_has(mix[i], AWARE_LOOP_REVERBERATION)) {
            if (mix_rv >= 0) return AWARE_E_BADARG;            // one reverberation chain per mixture: aware_embed_buffer 13 is its responses
            mix_rv = i;
        }
    }
    if (sum > 1.0 + 1e-6) return AWARE_E_BADARG;
    loop_mix_thresholds(w, n_chains, thr);
    return AWARE_OK;
}

// the two byte counts of the C ABI, from the dimensions alone
inline size_t loop_chain_workspace_bytes(const LoopDims& d, const aware_loop_attack_ex* attacks, int n_attacks) {
    if (!attacks || n_attacks < 1 || n_attacks > kMaxLoopAttacks) return 0;
    LoopChainState la;
    if (parse_loop_chain(d, attacks, n_attacks, true, la) == AWARE_E_BADARG) size_refused_chain(attacks, n_attacks, la);
    Carver c(nullptr, 0);
    carve_loop_chain(c, d, la);
    return c.off;
}
inline size_t loop_mixture_workspace_bytes(const LoopDims& d, const aware_loop_chain* chains, int n_chains) {
    LoopChainState shared, mix[kMaxLoopChains];
    unsigned long long thr[kMaxLoopChains];
    int rv = -1, *choice = nullptr;
    const int rc = parse_loop_mixture(d, chains, n_chains, mix, thr, rv);
    if (rc != AWARE_OK && rc != AWARE_E_UNSUPPORTED) return 0;
    Carver c(nullptr, 0);
    carve_loop_mixture(c, d, shared, mix, n_chains, choice);
    return c.off;
}

}  // namespace aware
