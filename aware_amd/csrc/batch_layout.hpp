// The host arithmetic of a batch (aware_batch_create, aware_batch_create_for_plan): the per-clip tables both routes share, and
// the card route's run lengths and workgroup tables.  Plain C++, no HIP header: tests/host_sim/batch_layout_check.cpp runs it on
// the CPU.  The geometry constants (kHop, kStreamWaves, kSynthBlocks) keep their one definition in the kernels' headers.
#pragma once
#include <algorithm>
#include <vector>

namespace aware {

// ---- both routes ----
struct BatchLayout {
    std::vector<int> in_off, T, frame_off, pool_off, out_off, out_len, pc_in;
    std::vector<int> order;           // clips longest first (dispatch order of the ragged GEMM: short clips fill the tail)
    int NF = 0, NP = 0, NS = 0, max_frames = 0, max_len = 0;
    int pstride = 0;                  // partial maxima per clip: the most 4096-sample pieces any input clip has
    int uniform_tp = 0;               // pooled frames per clip when all clips agree (else 0)
};
// Clip i: n_samples[i] samples at in_offsets[i] (null: packed), T = 1 + n / hop frames, hop (T - 1) samples of output.
// False when a clip is not longer than min_len_exclusive (torch.stft's reflect padding needs n > n_fft/2).
inline bool batch_layout(const int* n_samples, const int* in_offsets, int B, int hop, int min_len_exclusive, BatchLayout& L) {
    for (int i = 0; i < B; ++i)
        if (n_samples[i] <= min_len_exclusive) return false;
    L.in_off.resize(B); L.T.resize(B); L.out_off.resize(B); L.out_len.resize(B); L.pc_in.resize(B);
    L.frame_off.assign(B + 1, 0); L.pool_off.assign(B + 1, 0);
    long acc = 0;
    L.pstride = 1;
    for (int i = 0; i < B; ++i) {
        const int n = n_samples[i], T = 1 + n / hop;
        L.in_off[i] = in_offsets ? in_offsets[i] : (int)acc;
        acc += n;
        L.T[i] = T;
        L.frame_off[i + 1] = L.frame_off[i] + T;
        L.pool_off[i + 1] = L.pool_off[i] + ((T / 2 + 31) & ~31);   // floor(T / 2) pooled rows, 32-aligned per clip
        L.out_off[i] = hop * (L.frame_off[i] - i);
        L.out_len[i] = hop * (T - 1);
        L.pc_in[i] = (n + 4095) / 4096;
        L.max_frames = std::max(L.max_frames, T);
        L.max_len = std::max(L.max_len, n);
        L.pstride = std::max(L.pstride, L.pc_in[i]);
    }
    L.NF = L.frame_off[B];
    L.NP = L.pool_off[B];
    L.NS = hop * (L.NF - B);
    L.uniform_tp = L.T[0] / 2;
    for (int i = 1; i < B; ++i)
        if (L.T[i] / 2 != L.uniform_tp) L.uniform_tp = 0;
    L.order.resize(B);
    for (int i = 0; i < B; ++i) L.order[i] = i;
    std::stable_sort(L.order.begin(), L.order.end(), [&](int x, int y) { return L.T[x] > L.T[y]; });
    return true;
}

// ---- the general route ----
// 4096-sample pieces of each clip's output (the partial maxima of the synthesis side)
inline std::vector<int> pc_out_for(const std::vector<int>& out_len) {
    std::vector<int> pc(out_len.size());
    for (size_t i = 0; i < pc.size(); ++i) pc[i] = (out_len[i] + 4095) / 4096;
    return pc;
}

// ---- the card route: what it adds to the layout of its batch ----
struct CardRuns {
    int synth_run = 0;                // hop blocks per synthesis run: 12 / 8 / 6 / 4, or kSynthBlocks
    int an_run = 0;                   // frames per analysis run
    std::vector<int> pc_syn, an_wg, syn_wg;
};
// The exclusion: runs of `run` hop blocks would cut a clip of nb blocks into several segments of fewer than 3 blocks.  The
// staged adjoint folds the reflect pads inside the first / last segment, which takes 3 blocks.
inline bool run_cuts_short_segments(int nb, int run) {
    const int ns = (nb + run - 1) / run;
    return ns > 1 && nb / ns < 3;
}
// run length of the synthesis kernels (one wave of the streaming kernels per run): the longest of 16 / 12 / 8 / 6 / 4
// hop blocks that still gives ~16 waves per CU; a run of r blocks transforms r + 3 frames, so short runs cost more
// arithmetic and are only worth it while the chip would otherwise idle
// (measured, 3 s clips, us synthesis / adjoint: B = 256: 16 66/66, 12 65/64, 8 77/75; B = 128: 12 43/47, 8 40/42, 6 39/42,
// 4 51/52; B = 64: 8 31/30, 6 28/28, 4 28/28).  longest: kSynthBlocks, kept only where the exclusion bars every other length
inline int synth_run_for(const int* n_samples, int B, int hop, int longest) {
    int run = longest;
    for (int rb : {12, 8, 6, 4}) {          // (16 never measured better than 12)
        long runs = 0;
        bool ok = true;
        for (int i = 0; i < B; ++i) {
            runs += (n_samples[i] / hop + rb - 1) / rb;
            ok = ok && !run_cuts_short_segments(n_samples[i] / hop, rb);
        }
        if (!ok) continue;
        run = rb;
        if (runs >= 4096) break;
    }
    return run;
}
// synthesis runs of each clip (its partial maxima on the loop's signal layout): at least one
inline std::vector<int> pc_syn_for(const std::vector<int>& T, int synth_run) {
    std::vector<int> pc(T.size());
    for (size_t i = 0; i < pc.size(); ++i) pc[i] = std::max(1, (T[i] - 1 + synth_run - 1) / synth_run);
    return pc;
}
// frames per analysis run: the longest R in [4, 12] that still gives 4096 waves; for a uniform batch then the nearest
// shorter R whose run count per clip is a multiple of the waves of a workgroup (measurements: dsp_stream.hip)
inline int analysis_run_for(const std::vector<int>& T, int stream_waves) {
    // (runs longer than 12 frames measured slower even when the chip has waves to spare: B = 256 x 3 s, analysis / adjoint
    //  67 / 118 us at R = 12 against 69 / 136 at R = 16)
    constexpr int kAnalysisMaxRun = 12;
    auto total_runs = [&](int r) { long t = 0; for (int Ti : T) t += (Ti + r - 1) / r; return t; };
    int R = 4;
    for (int cand = kAnalysisMaxRun; cand >= 4; --cand)
        if (total_runs(cand) >= 4096) { R = cand; break; }
    bool same = true;
    for (int Ti : T) same = same && Ti == T[0];
    if (same)
        for (int cand = R; cand >= 4 && cand >= R - 3; --cand)
            if (((T[0] + cand - 1) / cand) % stream_waves == 0) { R = cand; break; }
    return R;
}
// streaming DSP kernels: one workgroup = stream_waves runs of one clip; flat tables (clip << 12 | workgroup within the clip) so
// that a ragged batch launches exactly the workgroups that have work.  Left empty where the packing cannot hold the batch.
inline void stream_wg_tables(const BatchLayout& L, CardRuns& C, int stream_waves) {
    const int B = (int)L.T.size();
    if (!(B < (1 << 19) && L.max_frames / 4 < 4096 * stream_waves)) return;
    for (int i = 0; i < B; ++i) {
        const int ra = (L.T[i] + C.an_run - 1) / C.an_run, rs = C.pc_syn[i];
        for (int w = 0; w < (ra + stream_waves - 1) / stream_waves; ++w) C.an_wg.push_back((i << 12) | w);
        for (int w = 0; w < (rs + stream_waves - 1) / stream_waves; ++w) C.syn_wg.push_back((i << 12) | w);
    }
}
// ... and raises L.pstride to the most synthesis runs a clip has, so that one stride serves both signal layouts
inline void card_runs(const int* n_samples, int hop, int stream_waves, int longest_synth_run, BatchLayout& L, CardRuns& C) {
    C.synth_run = synth_run_for(n_samples, (int)L.T.size(), hop, longest_synth_run);
    C.pc_syn = pc_syn_for(L.T, C.synth_run);
    for (int p : C.pc_syn) L.pstride = std::max(L.pstride, p);
    C.an_run = analysis_run_for(L.T, stream_waves);
    stream_wg_tables(L, C, stream_waves);
}

}  // namespace aware
