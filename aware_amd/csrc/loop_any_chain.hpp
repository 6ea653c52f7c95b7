// The host-only logic of the general route's attack chains (aware_embed_set_general_chain): the chain's
// state, the parser with every AWARE_E_BADARG / AWARE_E_UNSUPPORTED of the setter, and the carving of its workspace.  Plain
// C++: no HIP header and no HIP call, so tests/host_sim/general_chain_check.cpp runs it on the CPU.
//
// The general route serves the kinds that do not split a chain (loop_limits.hpp: gaussian noise, sample suppression, gain
// envelope): diagonal operators on the signal, which need nothing of the card's hop-block layout.  Its kernels
// (loop_any_chain.hip) work on a partition of their own: a clip of Ny samples is cut into ceil(Ny / kGenChainPiece) pieces,
// one workgroup each, and everything a clip needs as a whole (maxima, sums of squares, dot products) is exchanged as one
// partial per piece.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "loop_chain.hpp"

namespace aware {

// Samples per piece.  At most kEnvSpan (loop_gain.hpp), so that a workgroup's envelope table holds every breakpoint it meets;
// a multiple of 4, so that a thread's four samples are one Philox quad of the clip (loop_any_chain.hip asserts both)
constexpr int kGenChainPiece = 3072;
inline int gen_chain_pieces(int n) { return std::max(1, (n + kGenChainPiece - 1) / kGenChainPiece); }

struct GenChainState {
    int n = 0;                                // 0: the loop issues exactly the launches of the plain general route
    int kind[kMaxLoopAttacks] = {0}, k[kMaxLoopAttacks] = {0};
    double inv_snr[kMaxLoopAttacks] = {0};
    float prob[kMaxLoopAttacks] = {0};
    int p_lo[kMaxLoopAttacks] = {0}, p_hi[kMaxLoopAttacks] = {0};
    float floor[kMaxLoopAttacks] = {0};
    int pieces = 0;                           // pieces of the longest clip: the stride of the partial arrays
    float* z = nullptr;                       // [NS] the attacked signal
    unsigned long long* pmaxZ = nullptr;      // [B][pieces] partial maxima of |z|
    double* psq = nullptr;                    // [kMaxLoopAttacks][B][pieces] partial sums of x^2 in front of noise entry j
    double* pdotA = nullptr;                  // [B][pieces] partial sums of dL/da * a, a = N(N(z))
    double* pdotX = nullptr;                  // [B][pieces] partial sums of dL/dx * x, x = N(N(yraw))
    unsigned* seeds = nullptr;                // [B]
};

inline bool gen_chain_kind_served(int kind) {
    return kind == AWARE_LOOP_GAUSSIAN_NOISE || kind == AWARE_LOOP_SAMPLE_SUPPRESSION || kind == AWARE_LOOP_GAIN_ENVELOPE;
}

// The entries into the state: what the card's parser (parse_loop_chain, ex) calls a bad argument is AWARE_E_BADARG here too,
// more than kMaxLoopAttacks entries included; a well-formed entry of a kind this route does not serve, and a suppression
// that does not fit into every clip, are AWARE_E_UNSUPPORTED.  No buffer touched
inline int parse_gen_chain(const LoopDims& d, const aware_loop_attack_ex* attacks, int n_attacks, GenChainState& g) {
    LoopChainState la;
    const int rc = parse_loop_chain(d, attacks, n_attacks, true, la);
    if (rc == AWARE_E_BADARG) return rc;
    for (int j = 0; j < n_attacks; ++j)
        if (!gen_chain_kind_served(attacks[j].kind)) return AWARE_E_UNSUPPORTED;
    if (rc) return rc;
    g.n = n_attacks;
    for (int j = 0; j < kMaxLoopAttacks; ++j) {
        const bool in = j < n_attacks;
        g.kind[j] = in ? la.kind[j] : 0; g.k[j] = in ? la.k[j] : 0; g.inv_snr[j] = in ? la.inv_snr[j] : 0.0;
        g.prob[j] = in ? la.prob[j] : 0.f; g.p_lo[j] = in ? la.p_lo[j] : 0; g.p_hi[j] = in ? la.p_hi[j] : 0;
        g.floor[j] = in ? la.floor[j] : 0.f;
    }
    return AWARE_OK;
}

// the chain's workspace, whatever its entries are: the partial arrays follow the longest clip's pieces
inline void carve_gen_chain(Carver& c, const LoopDims& d, GenChainState& g) {
    g.pieces = gen_chain_pieces(*std::max_element(d.out_len, d.out_len + d.B));
    const size_t np = (size_t)d.B * g.pieces;
    g.z = c.take<float>(d.NS);
    g.pmaxZ = c.take<unsigned long long>(np);
    g.psq = c.take<double>(np * kMaxLoopAttacks);
    g.pdotA = c.take<double>(np);
    g.pdotX = c.take<double>(np);
    g.seeds = c.take<unsigned>(d.B);
}

// the byte count of the C ABI from the dimensions alone: 0 for what the setter calls a bad argument
inline size_t gen_chain_workspace_bytes(const LoopDims& d, const aware_loop_attack_ex* attacks, int n_attacks) {
    GenChainState g;
    if (d.B < 1 || !d.out_len || parse_gen_chain(d, attacks, n_attacks, g) == AWARE_E_BADARG) return 0;
    Carver c(nullptr, 0);
    carve_gen_chain(c, d, g);
    return c.off;
}

}  // namespace aware
