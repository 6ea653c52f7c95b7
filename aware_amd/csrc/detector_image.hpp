// The host arithmetic of a detector's parameters (aware_detector_create*, aware_detector_update): what a create call may ask
// for, the padded f32 image of mel basis, weights and biases, the two sparse mel forms, and where every packed operand sits.
// Plain C++, no HIP header: tests/host_sim/detector_image_check.cpp runs it on the CPU.  The kernels' constants (kFS, kMelTapsA,
// kMelTapsB, kMaxTapKernel, kMaxTapStride, kMinPool, kMaxPool) keep their one definition in the kernels' headers and the
// byte-count and support rules theirs in the GEMM files: both arrive as arguments.
#pragma once
#include <stddef.h>
#include <string.h>

#include <vector>

#include "../../include/aware_hip.h"

namespace aware {

// the widest last block (payloads of up to 512 bits), the largest mel bank and hidden width, the deepest network
constexpr int kMaxOutChannels = 1024;
constexpr int kMaxMels = 512;
constexpr int kMaxHidden = 4096;
constexpr int kMaxLayers = 33;
// The storage rule: the channel count layer boundary i (0 = the mel bank, n_layers = the last block) is stored with, for the
// caller's count C.  The only place that knows the padding.
//  - i = n_layers (C = 2 * payload bits): C itself where the read-out kernels for C <= 64 take it (a multiple of 4), C
//    rounded up to a multiple of 4 below that, and above 64 C rounded up to a multiple of 128 so that the conv-block kernels
//    take the block and the wide read-out (launch_readout_wide) reads it out;
//  - i < n_layers (mel bank and hidden widths): a multiple of 4 as is, else rounded up to a multiple of 4 up to 64 and to a
//    multiple of 128 above, so that the fused conv-block kernels take the block.
// Stored widths are multiples of 4 (the f32 GEMMs load K in float4).  Padding channels have zero weights, zero bias, zero
// weight columns in the next block and zero melT rows (and scale 0, shift 0 for BatchNorm): through every norm and
// activation they stay exactly 0 and their gradient is 0.
inline int stored_channels(int i, int n_layers, int C) {
    if (i < n_layers && C % 4 == 0) return C;
    if (C <= 64) return (C + 3) & ~3;
    return (C + 127) & ~127;
}

// ---- what a create call decides ----
struct DetectorSpec {
    int n_mels = 0, n_layers = 0;
    const int* channels = nullptr;               // the caller's [n_layers + 1]: n_mels, hidden widths, 2 * payload bits
    const aware_detector_arch* arch = nullptr;   // null: the model card's blocks and read-out (aware_detector_create only)
    bool arch_required = false;
    int kernel_size = 1, stride = 1, padding = 0;   // every block's Conv1d; other than 1 / 1 / 0: temporal convolutions
    int pool_size = 2, pool_stride = 2;             // the initial pool; other than 2 / 2: a pooled detector
    bool taps() const { return kernel_size != 1 || stride != 1 || padding != 0; }
    bool pooled() const { return pool_size != 2 || pool_stride != 2; }
    int stored(int i) const { return stored_channels(i, n_layers, channels[i]); }
};
struct DetectorLimits { int max_tap_kernel, max_tap_stride, min_pool, max_pool; };
// an aware_detector_arch with its enum values in range and, for BatchNorm, the folded map of every block
inline bool arch_ok(const aware_detector_arch* arch, int n_layers) {
    if (!arch) return false;
    if (arch->activation < AWARE_ACT_RELU || arch->activation > AWARE_ACT_SWISH) return false;
    if (arch->norm < AWARE_NORM_INSTANCE || arch->norm > AWARE_NORM_NONE) return false;
    if (arch->final_activation < AWARE_FINAL_RELU || arch->final_activation > AWARE_FINAL_SIGMOID) return false;
    if (arch->norm == AWARE_NORM_BATCH) {
        if (!arch->norm_scale || !arch->norm_shift || n_layers < 1 || n_layers > kMaxLayers) return false;
        for (int l = 0; l < n_layers; ++l)
            if (!arch->norm_scale[l] || !arch->norm_shift[l]) return false;
    }
    return true;
}
// AWARE_OK, or the code the create call returns.  One order for every entry point: the pool (arguments, then support), the
// convolution (the same; 2 * padding <= kernel_size - 1, so kernel 1 / stride 1 takes padding 0 only), the architecture, the
// pointers (pointers_ok: out, plan, mel basis and weights), the plan (plan_ok: not a general plan made for the transforms alone
// or with a band outside bins 0..n_fft/2), the sizes.
inline int detector_spec_check(const DetectorSpec& s, const DetectorLimits& lim, bool pointers_ok, bool plan_ok) {
    if (s.pool_size < 1 || s.pool_stride < 1) return AWARE_E_BADARG;
    if (s.pool_size < lim.min_pool || s.pool_size > lim.max_pool || s.pool_stride < lim.min_pool || s.pool_stride > lim.max_pool)
        return AWARE_E_UNSUPPORTED;
    if (s.kernel_size < 1 || s.stride < 1 || s.padding < 0) return AWARE_E_BADARG;
    if (s.kernel_size > lim.max_tap_kernel || s.stride > lim.max_tap_stride || 2 * s.padding > s.kernel_size - 1)
        return AWARE_E_UNSUPPORTED;
    if (s.arch_required && !arch_ok(s.arch, s.n_layers)) return AWARE_E_BADARG;
    if (!pointers_ok || !s.channels) return AWARE_E_BADARG;
    if (!plan_ok) return AWARE_E_UNSUPPORTED;
    if (s.n_mels < 1 || s.n_mels > kMaxMels || s.n_layers < 1 || s.n_layers > kMaxLayers || s.channels[0] != s.n_mels)
        return AWARE_E_UNSUPPORTED;
    const int cl = s.channels[s.n_layers];
    if (cl % 2 || cl < 2 || cl > kMaxOutChannels) return AWARE_E_UNSUPPORTED;
    for (int i = 1; i < s.n_layers; ++i)
        if (s.channels[i] < 1 || s.channels[i] > kMaxHidden) return AWARE_E_UNSUPPORTED;
    return AWARE_OK;
}

// ---- the f32 image ----
// the band of the plan the detector is created for: bins lo .. lo + nband - 1 of n_fft / 2 + 1, `stride` floats per band row;
// general: a general plan (dense mel operands only: the tap forms belong to the card kernels)
struct DetectorBand { int lo, nband, stride, n_fft; bool general; };
// With Mp = stored(0), S = band.stride, K = kernel_size and, per block l, ci = stored(l), co = stored(l + 1):
//   melT [Mp][S]: the band's columns of the mel basis, melT[j][f] = mel_basis[j][lo + f] for f < nband -- only the in-band
//                 columns ever multiply non-zero magnitudes (multibit_embedder.py:104, multibit_detector.py:34-37 zero the rest);
//   melB [S][Mp]: its transpose;
//   then per block w [co][K ci] with column j ci + c = tap j of input channel c (the caller's weights[l] is [rows][uci][K] for
//   its own counts), wT [K ci][co] its transpose, and the bias [co] (zero where biases or biases[l] is null).
// Padding rows and columns, and the columns beyond nband, are zero.
struct DetectorImage {
    std::vector<float> h;
    size_t o_melT = 0, o_melB = 0;
    std::vector<size_t> o_w, o_wT, o_b;
};
inline DetectorImage detector_image(const DetectorSpec& s, const DetectorBand& band, const float* mel_basis,
                                    const float* const* weights, const float* const* biases) {
    const int Mp = s.stored(0), S = band.stride, K = s.kernel_size, nbins = band.n_fft / 2 + 1;
    DetectorImage im;
    im.o_melB = (size_t)Mp * S;
    im.h.assign(2 * im.o_melB, 0.f);
    for (int j = 0; j < s.n_mels; ++j)
        for (int f = 0; f < band.nband; ++f)
            im.h[(size_t)j * S + f] = im.h[im.o_melB + (size_t)f * Mp + j] = mel_basis[(size_t)j * nbins + band.lo + f];
    for (int l = 0; l < s.n_layers; ++l) {
        const int ci = s.stored(l), co = s.stored(l + 1), kc = K * ci, uci = s.channels[l], rows = s.channels[l + 1];
        const size_t o_w = im.h.size(), o_wT = o_w + (size_t)kc * co, o_b = o_wT + (size_t)kc * co;
        im.o_w.push_back(o_w); im.o_wT.push_back(o_wT); im.o_b.push_back(o_b);
        im.h.resize(o_b + co, 0.f);
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < uci; ++c)
                for (int j = 0; j < K; ++j)
                    im.h[o_w + (size_t)r * kc + (size_t)j * ci + c] = im.h[o_wT + ((size_t)j * ci + c) * co + r] =
                        weights[l][((size_t)r * uci + c) * K + j];
        if (biases && biases[l]) memcpy(&im.h[o_b], biases[l], rows * sizeof(float));
    }
    return im;
}

// ---- the two sparse forms of a 128-filter bank on the card's band layout ----
struct MelTapShape { int fs, taps_a, taps_b; };   // kFS, kMelTapsA, kMelTapsB
// sparse: every band column has at most two non-zero filters, and they are adjacent (any triangular bank).  Column f is then
//   the two taps tw[2 f], tw[2 f + 1] at filters tm[f], tm[f] + 1, with tm[f] <= n_mels - 2: a column whose only filter is the
//   last one carries it in the second tap.
// runs: every filter m is besides non-zero in at most taps_a (m < 64) / taps_b adjacent columns: fw[m][taps_b] holds them from
//   column fs[m] on, with fs[m] <= fs - taps_b so that the run stays inside the row.
// Empty columns and empty filters keep zero entries.  A bank of another size, another band stride or a general plan: neither.
struct MelForms {
    bool sparse = false, runs = false;
    std::vector<float> tw, fw;
    std::vector<unsigned char> tm, fs;
};
inline MelForms mel_forms(const DetectorSpec& s, const DetectorBand& band, const DetectorImage& im, const MelTapShape& t) {
    const int n_mels = s.n_mels, Mp = s.stored(0), S = band.stride;
    const float* melT = im.h.data() + im.o_melT;
    const float* melB = im.h.data() + im.o_melB;
    MelForms m;
    m.tw.assign(2 * (size_t)t.fs, 0.f); m.tm.assign(t.fs, 0);
    m.fw.assign((size_t)128 * t.taps_b, 0.f); m.fs.assign(128, 0);
    m.sparse = n_mels == 128 && S == t.fs && !band.general;
    for (int f = 0; f < band.nband && m.sparse; ++f) {
        int first = -1, count = 0, lastnz = -1;
        for (int j = 0; j < n_mels; ++j)
            if (melB[(size_t)f * Mp + j] != 0.f) { if (first < 0) first = j; lastnz = j; ++count; }
        if (count == 0) continue;
        if (count > 2 || lastnz - first > 1) { m.sparse = false; break; }
        const int m1 = first < n_mels - 1 ? first : n_mels - 2;
        m.tm[f] = (unsigned char)m1;
        m.tw[2 * f] = melB[(size_t)f * Mp + m1];
        m.tw[2 * f + 1] = melB[(size_t)f * Mp + m1 + 1];
    }
    m.runs = m.sparse;
    for (int j = 0; j < n_mels && m.runs; ++j) {
        int first = -1, lastnz = -1;
        for (int f = 0; f < band.nband; ++f)
            if (melT[(size_t)j * S + f] != 0.f) { if (first < 0) first = f; lastnz = f; }
        if (first < 0) continue;
        const int taps = j < 64 ? t.taps_a : t.taps_b;
        const int start = first <= t.fs - t.taps_b ? first : t.fs - t.taps_b;
        if (lastnz - start >= taps) { m.runs = false; break; }
        m.fs[j] = (unsigned char)start;
        for (int k = 0; k < taps; ++k) m.fw[(size_t)j * t.taps_b + k] = melT[(size_t)j * S + start + k];
    }
    return m;
}

// ---- the packed operands ----
// the GEMM files' rules: bytes of a bf16x3 fragment image and of an f16 two-term image of [N][K], and the shapes the f16
// two-term kernel (nwm, N, K, lda) and the fused read-out (nwm, ci, C) serve
struct PackRules {
    size_t (*x3_packed_bytes)(int N, int K);
    size_t (*h2_packed_bytes)(int N, int K);
    bool (*gemm_clip_h2_supported)(int nwm, int N, int K, int lda);
    bool (*readout_x3_supported)(int nwm, int ci, int C);
};
// one operand [N][K]: whether it has a packed image, and the image's byte offset in its allocation
struct PackSlot { bool on = false; size_t off = 0; int N = 0, K = 0; };
// hands out consecutive slots of one allocation, each aligned to `align` bytes
struct PackTaker {
    size_t (*bytes)(int N, int K);
    size_t align, total = 0;
    PackSlot take(bool on, int N, int K) {
        const PackSlot t{on, total, N, K};
        if (on) total += (bytes(N, K) + align - 1) / align * align;
        return t;
    }
};
// bf16x3 fragment images (gemm_x3.hip), one allocation in this order: per block w [co][K ci] where co % 128 == 0 and
//   K ci % 64 == 0, then wT under the mirrored condition; melT [Mp][S] where Mp % 128 == 0 and melB [S][Mp] where Mp % 64 == 0
//   (always for 128 bands); the fused read-out's pair, for 1x1 blocks behind the (2, 2) pool, at least two blocks and a last
//   block the read-out takes: `last` = the last block's w with its rows zero-padded to colp = 16 ceil(col / 16), [colp][cil],
//   and `lastT` = its transpose with the columns zero-padded to 64, [cil][64] -- both here as host arrays, ready to pack.
// f16 two-term images (gemm_h2.hip), another allocation, 256-byte aligned: per block wh2 [co][ci] then wTh2 [ci][co] where the
//   kernel takes the shape.  They serve the fused conv blocks only: none for temporal convolutions or another pool.
struct PackedLayout {
    std::vector<PackSlot> w, wT, wh2, wTh2;
    PackSlot melT, melB, last, lastT;
    size_t x3_total = 0, h2_total = 0;
    std::vector<float> last_rows, lastT_rows;
};
inline PackedLayout packed_layout(const DetectorSpec& s, const DetectorBand& band, const DetectorImage& im, const PackRules& r) {
    const int nl = s.n_layers, K = s.kernel_size, Mp = s.stored(0), S = band.stride;
    const bool fused = !s.taps() && !s.pooled();
    PackedLayout L;
    PackTaker x3{r.x3_packed_bytes, 1}, h2{r.h2_packed_bytes, 256};
    for (int l = 0; l < nl; ++l) {
        const int ci = s.stored(l), co = s.stored(l + 1), kc = K * ci;
        L.w.push_back(x3.take(co % 128 == 0 && kc % 64 == 0, co, kc));
        L.wT.push_back(x3.take(kc % 128 == 0 && co % 64 == 0, kc, co));
        L.wh2.push_back(h2.take(fused && r.gemm_clip_h2_supported(1, co, ci, ci), co, ci));
        L.wTh2.push_back(h2.take(fused && r.gemm_clip_h2_supported(1, ci, co, co), ci, co));
    }
    L.melT = x3.take(Mp % 128 == 0, Mp, S);
    L.melB = x3.take(Mp % 64 == 0, S, Mp);
    const int cil = s.stored(nl - 1), col = s.stored(nl), colp = 16 * ((col + 15) / 16);
    const bool ro = fused && nl >= 2 && r.readout_x3_supported(1, cil, col);
    L.last = x3.take(ro, colp, cil);
    L.lastT = x3.take(ro, cil, 64);
    L.x3_total = x3.total; L.h2_total = h2.total;
    if (ro) {
        L.last_rows.assign((size_t)colp * cil, 0.f);
        L.lastT_rows.assign((size_t)cil * 64, 0.f);
        for (int row = 0; row < col; ++row)
            for (int c = 0; c < cil; ++c)
                L.last_rows[(size_t)row * cil + c] = L.lastT_rows[(size_t)c * 64 + row] = im.h[im.o_w[nl - 1] + (size_t)row * cil + c];
    }
    return L;
}

// ---- BatchNorm (eval mode, folded): per block the scale [co] then the shift [co] ----
// padding channels (stored_channels) get scale 0 and shift 0: their pre-activation is 0 and their output act(0) = 0 for every
// block activation.  They are never read out and their gradient is zero.
struct NormImage { std::vector<float> h; std::vector<size_t> o_scale, o_shift; };
inline NormImage norm_image(const DetectorSpec& s) {
    NormImage n;
    for (int l = 0; l < s.n_layers; ++l) {
        const size_t o = n.h.size(), co = s.stored(l + 1), rows = s.channels[l + 1];
        n.o_scale.push_back(o); n.o_shift.push_back(o + co);
        n.h.resize(o + 2 * co, 0.f);
        memcpy(&n.h[o], s.arch->norm_scale[l], rows * sizeof(float));
        memcpy(&n.h[o + co], s.arch->norm_shift[l], rows * sizeof(float));
    }
    return n;
}

}  // namespace aware
