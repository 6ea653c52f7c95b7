// csrc/detector_image.hpp on the CPU (no HIP): reads one case per line, every number an integer,
//   stored
//   check  <spec> <arch_required> <arch_mode> <activation> <norm> <final_activation> <pointers_ok> <plan_ok>
//   image  <spec> <lo> <nband> <stride> <n_fft> <general> <bias_mask> mel.. weights.. biases..
//   norm   <spec> scale.. shift..
// with <spec> = n_mels n_layers <count> channels[0 .. count - 1] kernel_size stride padding pool_size pool_stride (count 0: a
// null channels pointer); arch_mode 0: null, 1: null arrays, 2: arrays, 3: arrays whose last entries are null; bias_mask -1: a
// null biases pointer, else bit l set: biases[l] present (the values of every block are on the line all the same).  mel is
// [n_mels][n_fft / 2 + 1], weights per block [channels[l + 1]][channels[l]][kernel_size], then biases, scale and shift per block
// [channels[l + 1]].  Prints one JSON object per line.  Run by tests/test_detector_image_host.py.
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>

#include "../../aware_amd/csrc/detector_image.hpp"

using namespace aware;

// the kernels' constants as common.hpp and conv_taps.hpp define them (those headers need HIP)
constexpr MelTapShape kMelShape{256, 6, 12};    // kFS, kMelTapsA, kMelTapsB
constexpr DetectorLimits kLimits{7, 4, 2, 8};   // kMaxTapKernel, kMaxTapStride, kMinPool, kMaxPool
// stand-ins for the GEMM files' rules, restated in the test: byte counts that are no multiple of 256, an f16 rule that also
// checks that the row pitch handed over is K, a read-out rule
static size_t x3_bytes(int N, int K) { return (size_t)6 * N * K + 6; }
static size_t h2_bytes(int N, int K) { return (size_t)4 * N * K + 4 * N + 4; }
static bool h2_ok(int nwm, int N, int K, int lda) { return nwm == 1 && N % 128 == 0 && K % 64 == 0 && lda == K; }
static bool readout_ok(int nwm, int ci, int C) { return nwm == 1 && ci % 128 == 0 && C <= 48; }
constexpr PackRules kRules{x3_bytes, h2_bytes, h2_ok, readout_ok};

template <typename T> static void tab(const char* name, const std::vector<T>& v) {
    printf(", \"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) printf(i ? ",%.9g" : "%.9g", (double)v[i]);
    printf("]");
}
static void slot(const char* name, const PackSlot& t) {
    printf(", \"%s\": [%d,%zu,%d,%d]", name, (int)t.on, t.off, t.N, t.K);
}
static void slots(const char* name, const std::vector<PackSlot>& v) {
    printf(", \"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s[%d,%zu,%d,%d]", i ? "," : "", (int)v[i].on, v[i].off, v[i].N, v[i].K);
    printf("]");
}
static std::vector<float> floats(std::istream& in, size_t n) {
    std::vector<float> v(n);
    for (float& x : v) { long t = 0; in >> t; x = (float)t; }
    return v;
}
// one array per block, `per(l)` values each, and the pointers to them
struct Blocks {
    std::vector<std::vector<float>> v;
    std::vector<const float*> p;
    template <typename F> Blocks(std::istream& in, int nl, F per) {
        for (int l = 0; l < nl; ++l) v.push_back(floats(in, per(l)));
        for (auto& x : v) p.push_back(x.data());
    }
};

static void stored() {
    std::vector<int> hidden, last;
    for (int C = 1; C <= 4096; ++C) hidden.push_back(stored_channels(1, 3, C));
    for (int C = 2; C <= 1024; C += 2) last.push_back(stored_channels(3, 3, C));
    printf("{\"n\": 0");
    tab("hidden", hidden); tab("last", last);
    printf("}\n");
}

static void check(std::istream& in, DetectorSpec s) {
    int mode = 0, pointers_ok = 0, plan_ok = 0;
    aware_detector_arch a{};
    in >> s.arch_required >> mode >> a.activation >> a.norm >> a.final_activation >> pointers_ok >> plan_ok;
    const float one = 1.f;
    std::vector<const float*> arr(kMaxLayers, &one);
    if (mode == 3 && s.n_layers >= 1 && s.n_layers <= kMaxLayers) arr[s.n_layers - 1] = nullptr;
    if (mode >= 2) a.norm_scale = a.norm_shift = arr.data();
    if (mode) s.arch = &a;
    printf("{\"rc\": %d}\n", detector_spec_check(s, kLimits, pointers_ok != 0, plan_ok != 0));
}

static void image(std::istream& in, const DetectorSpec& s) {
    DetectorBand band{};
    int general = 0, bias_mask = 0;
    in >> band.lo >> band.nband >> band.stride >> band.n_fft >> general >> bias_mask;
    band.general = general != 0;
    const std::vector<float> mel = floats(in, (size_t)s.n_mels * (band.n_fft / 2 + 1));
    const Blocks w(in, s.n_layers, [&](int l) { return (size_t)s.channels[l + 1] * s.channels[l] * s.kernel_size; });
    Blocks b(in, s.n_layers, [&](int l) { return (size_t)s.channels[l + 1]; });
    for (int l = 0; l < s.n_layers; ++l)
        if (!(bias_mask >> l & 1)) b.p[l] = nullptr;
    const DetectorImage im = detector_image(s, band, mel.data(), w.p.data(), bias_mask < 0 ? nullptr : b.p.data());
    const MelForms m = mel_forms(s, band, im, kMelShape);
    const PackedLayout p = packed_layout(s, band, im, kRules);
    printf("{\"o_melT\": %zu, \"o_melB\": %zu, \"sparse\": %d, \"runs\": %d, \"x3_total\": %zu, \"h2_total\": %zu", im.o_melT, im.o_melB,
           (int)m.sparse, (int)m.runs, p.x3_total, p.h2_total);
    tab("h", im.h); tab("o_w", im.o_w); tab("o_wT", im.o_wT); tab("o_b", im.o_b);
    tab("tw", m.tw); tab("tm", m.tm); tab("fw", m.fw); tab("fs", m.fs);
    slots("x3_w", p.w); slots("x3_wT", p.wT); slot("x3_melT", p.melT); slot("x3_melB", p.melB);
    slot("x3_last", p.last); slot("x3_lastT", p.lastT);
    tab("last_rows", p.last_rows); tab("lastT_rows", p.lastT_rows);
    slots("h2_w", p.wh2); slots("h2_wT", p.wTh2);
    printf("}\n");
}

static void norm(std::istream& in, DetectorSpec s) {
    const Blocks scale(in, s.n_layers, [&](int l) { return (size_t)s.channels[l + 1]; });
    const Blocks shift(in, s.n_layers, [&](int l) { return (size_t)s.channels[l + 1]; });
    const aware_detector_arch a{0, AWARE_NORM_BATCH, 0, scale.p.data(), shift.p.data()};
    s.arch = &a;
    const NormImage n = norm_image(s);
    printf("{\"n\": %zu", n.h.size());
    tab("h", n.h); tab("o_scale", n.o_scale); tab("o_shift", n.o_shift);
    printf("}\n");
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "stored") { stored(); continue; }
        DetectorSpec s;
        int count = 0;
        in >> s.n_mels >> s.n_layers >> count;
        std::vector<int> ch(count);
        for (int& c : ch) in >> c;
        if (count) s.channels = ch.data();
        in >> s.kernel_size >> s.stride >> s.padding >> s.pool_size >> s.pool_stride;
        if (what == "check") check(in, s);
        else if (what == "image") image(in, s);
        else if (what == "norm") norm(in, s);
        if (!in) { fprintf(stderr, "short line: %s\n", what.c_str()); return 1; }
    }
    return 0;
}
