// Limits and kind numbers of the embed loop's attack chains and the mixture's gate: what the kernels (kernels.h, common.hpp) and
// the host-only chain logic (loop_chain.hpp) share.  Plain C++: no HIP header, no HIP call.
#pragma once

namespace aware {

constexpr int kMaxLoopChains = 8;
constexpr int kMaxLoopAttacks = 4;
constexpr int kLoopGaussianNoise = 0, kLoopSampleSuppression = 1, kLoopReverberation = 2, kLoopSpeedChange = 3, kLoopTimeStretch = 4,
              kLoopPitchShift = 5, kLoopPhaseVocoder = 6, kLoopDeleteSamples = 7, kLoopGainEnvelope = 8,
              kLoopBandFilter = 9, kLoopExcerpt = 10, kLoopTimeWarp = 11, kLoopFrequencyShift = 12;      // AWARE_LOOP_* of aware_hip.h

// THE KINDS, one row each, indexed by the kind's number.  splits: the kind needs launches of its own between two stages of
// element-wise entries (the one-split rule, loop_chain.hpp); the others run inside the stage kernels.  ex_only: only the _ex
// entry points and the mixture's setter accept it.  refused_rank: a refused chain is sized by the splitting entry of the lowest
// rank (size_refused_chain); -1 where the kind never decides.  The host twin is embedding/loop_attacks.py::TABLE.
struct LoopKindRow { bool splits, ex_only; int refused_rank; };
constexpr LoopKindRow kLoopKindTable[] = {
    {false, false, -1},      //  0 gaussian noise
    {false, false, -1},      //  1 sample suppression
    {true, true, 0},         //  2 reverberation
    {true, true, 3},         //  3 speed change
    {true, true, 2},         //  4 time stretch
    {true, true, 4},         //  5 pitch shift
    {true, true, 1},         //  6 phase vocoder
    {true, true, 5},         //  7 sample deletion
    {false, true, -1},       //  8 gain envelope
    {true, true, 6},         //  9 band filter
    {true, true, 7},         // 10 tiled excerpt
    {true, true, 8},         // 11 time warp
    {false, true, -1},       // 12 frequency shift: takes a stage of its own all the same, see kLoopStagedBeyond
};
constexpr int kLoopKinds = sizeof(kLoopKindTable) / sizeof(kLoopKindTable[0]);
static_assert(kLoopKinds == kLoopFrequencyShift + 1, "one row per kind");

// The `splits` column and the ranks are closed at the time warp: the suite records that the time warp is the last splitting
// kind (tests/test_loop_warp_host.py) and that the ranks of the splitting rows count from 0 without a gap.  A kind added since
// that needs launches of its own is listed here instead, in the order in which it was added, and is treated by the one-split
// rule, the carver and the stage dispatch exactly as a splitting row is; its rank where a refused chain is sized follows the
// table's last.  The host twin is embedding/loop_attacks.py::STAGED.
constexpr int kLoopStagedBeyond[] = {kLoopFrequencyShift};
constexpr int kLoopTableRanks = 9;        // the ranks 0..8 of the table
// whether the kind takes a stage of its own: a splitting row, or a kind of kLoopStagedBeyond
constexpr bool loop_kind_staged(int kind) {
    if (kLoopKindTable[kind].splits) return true;
    for (int k : kLoopStagedBeyond)
        if (k == kind) return true;
    return false;
}
// refused_rank of a kind with a stage of its own
constexpr int loop_staged_rank(int kind) {
    int i = 0;
    for (int k : kLoopStagedBeyond) {
        if (k == kind) return kLoopTableRanks + i;
        ++i;
    }
    return kLoopKindTable[kind].refused_rank;
}
static_assert(loop_kind_staged(kLoopFrequencyShift) && loop_staged_rank(kLoopFrequencyShift) == 9 && loop_staged_rank(kLoopTimeWarp) == 8 &&
              !loop_kind_staged(kLoopGainEnvelope), "");

// reverberation (loop_reverb_kernels.hip)
constexpr int kReverbMaxIr = 8192;        // taps
constexpr int kReverbBlock = 2048;        // output samples per block; the transform has 4096 points
constexpr int kReverbBins = 2056;         // complex values per spectrum row: bins 0..2048 and padding
constexpr int kReverbParts = 4;           // partitions of 2048 taps
constexpr int kReverbTwHalf = 1024;       // W_2048^j, j < 1024; then W_4096^k, k <= 2048, padded to kReverbBins
inline int reverb_blocks(int n) { return (n + kReverbBlock - 1) / kReverbBlock; }

constexpr int kSpeedMin = -13520, kSpeedMax = 17034;      // speed offsets: ceil / floor of 65536 (2^(-+400 / 1200) - 1)
constexpr int kStretchMin = -16384, kStretchMax = 21845;  // stretch offsets: ceil / floor of 65536 (0.75 - 1) and 65536 (4 / 3 - 1)

// gain envelope (loop_attack_kernels.hip, loop_gain_kernels.hip): samples between two breakpoints
constexpr int kEnvelopeMinPeriod = 64, kEnvelopeMaxPeriod = 1 << 20;

// band filter (loop_filter_kernels.hip): taps on either side of the centre; edges in units of 1 / 65536 cycle per sample
constexpr int kFilterHalf = 127, kFilterMaxEdge = 32767;

// tiled excerpt (loop_excerpt_kernels.hip): the shortest excerpt a chain may draw, in samples
constexpr int kExcerptMinLen = 1024;

// time warp (loop_warp_kernels.hip): samples between two breakpoints of the rate are 2^e, kWarpMinExp <= e <= kWarpMaxExp; a
// rate is (65536 + m) / 65536 with |m| <= D <= kWarpMaxDepth (a tenth either way)
constexpr int kWarpMinExp = 8, kWarpMaxExp = 20, kWarpMaxDepth = 6553;
// breakpoints of a clip of n samples at 2^e between them: the last position read is n - 1 + 2^e - 1, and the segment it lies
// in needs the breakpoint behind it
constexpr int warp_breakpoints(int n, int e) { return (int)(((long long)n + (1ll << e) - 1) >> e) + 2; }

// frequency shift (loop_shift_kernels.hip): the widest shift either way, in units of sr / 2^20 Hz: sr / 16.  Its Hilbert
// transformer has the band filter's kFilterHalf taps on either side
constexpr int kShiftMax = 65536;

// Attack mixtures: with `choice` set, a workgroup whose clip did not draw chain `chain` at this step returns at once
struct LoopGate {
    const int* choice = nullptr;          // [B] the chain clip b drew at this step, -1: none
    int chain = 0;
};

}  // namespace aware
