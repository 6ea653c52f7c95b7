// extern "C" entry points of libaware_hip (see include/aware_hip.h for the contract and the
// reference code each one replaces).  Host-side orchestration only: geometry tables,
// workspace carving, launch sequences, optional hipGraph capture of one optimiser iteration.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <algorithm>
#include <memory>
#include <vector>

#include "../../include/aware_hip.h"
#include "common.hpp"
#include "kernels.h"
#define AWARE_LOOP_CF cf
#include "loop_chain.hpp"
#include "loop_any_chain.hpp"
#include "batch_layout.hpp"
#include "detector_image.hpp"

using namespace aware;

static thread_local std::string g_last_err;

#define HIPCHK(expr)                                                                  \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) {                                                       \
            g_last_err = std::string(#expr) + ": " + hipGetErrorString(_e);           \
            return AWARE_E_HIP;                                                       \
        }                                                                             \
    } while (0)
#define LAUNCHCHK() HIPCHK(hipGetLastError())

// A handle under construction: every return between `new` and `*out = h.release()` destroys it with the object's own
// aware_*_destroy (each of which takes a half-built object: it frees what is not null)
template <auto Destroy> struct HandleDeleter { template <typename H> void operator()(H* h) const { Destroy(h); } };
template <typename H, auto Destroy> using Building = std::unique_ptr<H, HandleDeleter<Destroy>>;

// Optional per-launch timing of one optimiser iteration (aware_embed_profile): an event is
// recorded on the launch stream after every kernel; consecutive events bracket one kernel.
struct LaunchProfiler {
    hipStream_t st;
    std::vector<hipEvent_t> ev;
    std::vector<int> kind;
};
static thread_local LaunchProfiler* g_prof = nullptr;
static inline void prof_mark(int kind) {
    if (!g_prof) return;
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, g_prof->st);
    g_prof->ev.push_back(e);
    g_prof->kind.push_back(kind);
}
#define PROF(kind) prof_mark(kind)
// kernel kinds reported by aware_embed_profile
enum { K_SYNTH = 0, K_ANALYSIS = 1, K_GEMM = 2, K_MELNORM = 3, K_INLRELU = 4, K_HEAD = 5, K_SYNTH_ADJ = 6,
       K_ANALYSIS_ADJ = 7, K_MISC = 8, K_GEMM_CLIP_FWD = 9, K_GEMM_CLIP_BWD = 10, K_GEMM_X3_FWD = 11, K_GEMM_X3_BWD = 12 };

static int absmax_into_scratch(const float* in, const int* off, const int* len, int B, int max_len, void* scratch,
                               unsigned long long** pmax_out, int** pcount_out, int* ps_out, hipStream_t st);

// ---------------------------------------------------------------------------------------------
struct aware_plan {
    PlanDev dev;
    void* mem = nullptr;
    // general-geometry plans (stft_any.hip): every geometry other than the card's, or any geometry created with
    // AWARE_PLAN_GENERAL.  The transforms run on stft_any.hip, the embed / detect loop on the general route (loop_any.hip).
    // loop: created with AWARE_PLAN_GENERAL, which also opens the embed / detect loop on it; a plan that is general only
    // because its geometry is not the card's serves the transforms alone, and the loop's entry points refuse it with
    // AWARE_E_UNSUPPORTED before they read another argument.  band_ok: the band lies inside bins 0..n_fft/2 (a plan made for
    // the transforms may carry any band; the loop refuses it)
    int general = 0, loop = 0, band_ok = 1;
    int n_fft = kNfft, hop = kHop, win_length = kNfft, window = 0;
    GenPlanDev gdev;
    std::vector<float> w2h, envh;       // host copies of the squared window and the envelope tables (NOLA check)
};

// host tables and scalars: batch_layout.hpp's BatchLayout on both routes, CardRuns (runs, workgroup tables) on the card route
struct aware_batch : BatchLayout, CardRuns {
    int B = 0;
    std::vector<int> n;
    // device tables (one allocation)
    int* d_mem = nullptr;
    int *d_frame_off = nullptr, *d_pool_off = nullptr, *d_in_off = nullptr, *d_in_len = nullptr, *d_out_off = nullptr,
        *d_out_len = nullptr, *d_pc_in = nullptr, *d_pc_syn = nullptr;
    int *d_an_wg = nullptr, *d_syn_wg = nullptr;
    int* d_order = nullptr;
    // batch built by aware_batch_create_for_plan for a general plan: its geometry, whether every clip passes the NOLA
    // condition, and the frame buffer of the synthesis direction [NF][n_fft] floats
    int general = 0;
    int g_nfft = 0, g_hop = 0, g_win = 0, g_window = 0, nola_ok = 1;
    int* d_pc_out = nullptr;
    float* d_frames = nullptr;
};

struct aware_detector {
    int n_mels = 0, n_layers = 0, nbits = 0;
    int band_lo = 0, nband = 0;
    int stride = kFS;        // floats per band row of the plan the detector was created for
    int n_fft = kNfft;       // ... and its transform size: the mel basis handed over is [n_mels][n_fft/2 + 1]
    bool general = false;    // created for a general plan: dense mel operands only (the tap forms belong to the card kernels)
    // channel counts as the caller gave them (uch) and as stored (ch, stored_channels): ch[0] = Mp >= n_mels is the row
    // stride of the mel stage; padding channels have zero weights, bias and melT rows and get a zero gradient
    std::vector<int> uch, ch;
    int maxc = 0;
    float* mem = nullptr;
    float* melT = nullptr;   // [Mp][stride]  (Bt of the forward mel GEMM; rows n_mels .. Mp-1 zero)
    float* melB = nullptr;   // [stride][Mp]  (Bt of its data-gradient)
    std::vector<float*> w;    // [Cout][Cin]
    std::vector<float*> wT;   // [Cin][Cout]
    // the same two operands split into three bf16 planes in MFMA fragment order (gemm_x3.hip); null when the
    // shape is not served by that kernel
    std::vector<void*> wpk, wTpk;
    void* melTpk = nullptr;
    void* melBpk = nullptr;
    void* lastpk = nullptr;    // last conv, rows zero-padded to a multiple of 16 (read-out kernel)
    void* lastTpk = nullptr;   // its transpose [Cin][64], k zero-padded to 64
    void* pkmem = nullptr;
    // the conv blocks' two operands as f16 two-term images (gemm_h2.hip: planes + per-channel inverse scales)
    std::vector<void*> wh2, wTh2;
    void* h2mem = nullptr;
    std::vector<float*> bias;
    // the mel filter bank as two taps per band column (a triangular bank has at most two adjacent non-zero weights per bin):
    // melw [kFS] float2, melm [kFS] first tap's mel index (<= 126); null when the basis handed over is not of that form, the
    // bank is not 128 bands or the band has the wide layout (which takes the dense mel GEMMs)
    void* mel2mem = nullptr;
    float2* melw = nullptr;
    unsigned char* melm = nullptr;
    // ... and per filter as a short run of adjacent band columns (forward): melf_w [n_mels][kMelTapsB], melf_s [n_mels]; null
    // when a filter's support is longer than the folded analysis kernel takes (kMelTapsA / kMelTapsB columns)
    float* melf_w = nullptr;
    unsigned char* melf_s = nullptr;
    // architecture (aware_detector_arch).  card_arch: InstanceNorm + LeakyReLU(0.2) blocks and a tanh read-out, the model card's
    // network and the only one the fused kernels serve (conv-block epilogues, read-out, tail); every other detector takes the
    // staged route: plain GEMM + bias, launch_norm_act, launch_head
    bool card_arch = true;
    int act = kActLRelu, norm = kNormInstance, final_act = kActTanh;
    std::vector<float*> nscale, nshift;   // affine norm (BatchNorm1d in eval mode, folded): u = z * nscale[l][c] + nshift[l][c]
    float* normmem = nullptr;
    // temporal convolutions (aware_detector_create_conv with kernel_size / stride / padding other than 1 / 1 / 0; conv_taps.hpp):
    // every block is Conv1d over tk taps, stride ts, padding tp.  w[l] is then [Cout][tk Cin] (column j Cin + ci = tap j of
    // input channel ci), wT[l] its transpose and wpk / wTpk their packed forms: the operands of the plain GEMM on the unfolded
    // rows.  Such a detector is never card_arch: it runs the staged route in every block, whatever its activations are
    bool taps = false;
    int tk = 1, ts = 1, tp = 0;
    int max_cin = 0;         // the widest block input (stored), for the unfold scratch [NP][tk max_cin]
    // the initial pool between the mel stage and block 0 (aware_detector_create_pool; conv_taps.hpp: pool_rows): AvgPool1d(psize,
    // pstride).  Other than (2, 2) the detector is `pooled` and, like one of temporal convolutions, never card_arch: the mel
    // stage runs mel_pool_kernels.hip and every block the staged route on the clip's pool_rows rows -- the fused kernels, the
    // clip-form mel kernels and mel_front_x3 / mel_back_x3 all hold floor(T / 2)
    bool pooled = false;
    int psize = 2, pstride = 2;
};
// the rows a kernel behind `blocks` blocks of the detector works on
static TapRows det_rows(const aware_detector* d, int blocks) {
    TapRows r = d->taps ? TapRows{blocks, d->tk, d->ts, d->tp} : TapRows();
    r.psize = d->psize; r.pstride = d->pstride;
    return r;
}
// every clip keeps at least one row behind the pool and through every block (torch's avg_pool1d / conv1d raise where one does not)
static bool det_clips_ok(const aware_detector* d, const aware_batch* b) {
    if (!d->taps && !d->pooled) return true;
    for (int i = 0; i < b->B; ++i)
        if (conv_rows(pool_rows(b->T[i], d->psize, d->pstride), d->n_layers, d->tk, d->ts, d->tp) < 1) return false;
    return true;
}
static_assert(AWARE_ACT_RELU == kActRelu && AWARE_ACT_LEAKY_RELU == kActLRelu && AWARE_ACT_GELU == kActGelu &&
              AWARE_ACT_SWISH == kActSwish && AWARE_FINAL_TANH == kActTanh && AWARE_FINAL_SIGMOID == kActSigmoid &&
              AWARE_FINAL_RELU == kActRelu && AWARE_FINAL_LEAKY_RELU == kActLRelu && AWARE_FINAL_GELU == kActGelu &&
              AWARE_FINAL_SWISH == kActSwish, "activation enums");
static_assert(AWARE_NORM_INSTANCE == kNormInstance && AWARE_NORM_BATCH == kNormAffine && AWARE_NORM_NONE == kNormNone, "norm enums");
// whether the staged route keeps the pre-activation of every block for the backward (DetBufs::stash)
static bool det_needs_stash(const aware_detector* d) { return !d->card_arch && norm_act_needs_stash(d->norm, d->act); }

extern "C" int aware_version(void) { return 350; }
extern "C" const char* aware_last_hip_error(void) { return g_last_err.c_str(); }

// ---------------------------------------------------------------------------------------------
// ---- general-geometry tables (host) ----
static bool gen_nfft_supported(int n) { return n == 256 || n == 512 || n == 1024 || n == 2048 || n == 4096; }
static int gen_stride(int n_fft) { return (n_fft / 2 + 1 + 7) & ~7; }

// torch.hann_window / torch.hamming_window(win_length) (periodic), zero-padded to n_fft with left pad
// (n_fft - win_length) / 2 as torch.stft / torch.istft do; its square; the envelope tables of gen_env (kernels.h)
static void gen_host_tables(int N, int hop, int win, int window, std::vector<float>& w, std::vector<float>& w2,
                            std::vector<float>& env) {
    const double PI = 3.14159265358979323846;
    w.assign(N, 0.f);
    w2.assign(N, 0.f);
    const int lpad = (N - win) / 2;
    for (int i = 0; i < win; ++i) {
        const double c = cos(2 * PI * i / win);
        w[lpad + i] = (float)(window == 0 ? 0.5 - 0.5 * c : 0.54 - 0.46 * c);
    }
    for (int i = 0; i < N; ++i) w2[i] = w[i] * w[i];
    env.assign(N + hop + N / 2, 0.f);
    const int big = N / hop + 2;                               // any T with T*hop >= N
    for (int p = 0; p < N; ++p) env[p] = gen_env_loop(w2.data(), N, hop, p, big);
    for (int r = 0; r < hop; ++r) env[N + r] = gen_env_loop(w2.data(), N, hop, N + ((r - N % hop) % hop + hop) % hop, big);
    for (int q = 0; q < N / 2; ++q) env[N + hop + q] = gen_env_loop(w2.data(), N, hop, big * hop + q, big);
}

// torch.istft's NOLA condition for a clip of T frames: the envelope stays >= 1e-11 over the trimmed output
// [N/2, N/2 + hop (T - 1)).  Interior positions repeat with period hop, so one period of them is checked.
static bool gen_nola_ok(const float* env, const float* w2, int N, int hop, int T) {
    const int lo = N / 2, hi = N / 2 + hop * (T - 1);
    const bool tables = (long)T * hop >= N;
    for (int p = lo; p < hi; ++p) {
        if (tables && p == N + hop && p < T * hop) {
            p = T * hop - 1;
            continue;
        }
        if (!(gen_env(env, w2, N, hop, p, T) >= 1e-11f)) return false;
    }
    return true;
}

static int gen_validate(int n_fft, int hop, int win_length, int window) {
    if (!gen_nfft_supported(n_fft)) return AWARE_E_UNSUPPORTED;
    if (hop < 1 || hop > n_fft || win_length < 1 || win_length > n_fft || (window != 0 && window != 1)) return AWARE_E_BADARG;
    return AWARE_OK;
}

static int gen_plan_create(aware_plan** out, int n_fft, int hop, int win_length, int window, int band_lo_bin,
                           int band_hi_bin, int flags) {
    const int rc = gen_validate(n_fft, hop, win_length, window);
    if (rc != AWARE_OK) return rc;
    const int N = n_fft, M = N / 2;
    const double PI = 3.14159265358979323846;
    std::vector<float> w, w2, env;
    gen_host_tables(N, hop, win_length, window, w, w2, env);
    // device image (floats, every part 16-byte aligned): th [M/2] cf, twN [M + 1 -> M + 2] cf, window, window2, env
    std::vector<float> h;
    auto put = [&](const float* src, size_t n) {
        const size_t o = h.size();
        h.insert(h.end(), src, src + n);
        h.resize((h.size() + 3) & ~(size_t)3, 0.f);
        return o;
    };
    std::vector<float> th(M), twN(2 * (M + 2), 0.f);
    for (int j = 0; j < M / 2; ++j) {
        th[2 * j] = (float)cos(2 * PI * j / M);
        th[2 * j + 1] = (float)-sin(2 * PI * j / M);
    }
    for (int k = 0; k <= M; ++k) {
        twN[2 * k] = (float)cos(2 * PI * k / N);
        twN[2 * k + 1] = (float)-sin(2 * PI * k / N);
    }
    twN[0] = 1.f; twN[1] = 0.f;                   // exact at 0, -pi/2, -pi: DC and Nyquist come out purely real
    twN[M] = 0.f; twN[M + 1] = -1.f;
    twN[2 * M] = -1.f; twN[2 * M + 1] = 0.f;
    const size_t o_th = put(th.data(), th.size()), o_tw = put(twN.data(), twN.size());
    const size_t o_w = put(w.data(), w.size()), o_w2 = put(w2.data(), w2.size()), o_env = put(env.data(), env.size());
    Building<aware_plan, aware_plan_destroy> p(new aware_plan());
    if (hipMalloc(&p->mem, h.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(p->mem, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        g_last_err = "aware_plan_create: device tables";
        return AWARE_E_HIP;
    }
    const float* d = (const float*)p->mem;
    p->general = 1;
    p->loop = (flags & AWARE_PLAN_GENERAL) ? 1 : 0;
    p->n_fft = N; p->hop = hop; p->win_length = win_length; p->window = window;
    p->gdev.n_fft = N; p->gdev.hop = hop; p->gdev.stride = gen_stride(N);
    p->gdev.th = (const cf*)(d + o_th);
    p->gdev.twN = (const cf*)(d + o_tw);
    p->gdev.window = d + o_w;
    p->gdev.window2 = d + o_w2;
    p->gdev.env = d + o_env;
    // band rows of the loop: nband columns rounded up to whole 64-column chunks (K % 64 == 0 for the mel GEMMs, one wave
    // per chunk in loop_any.hip); 2112 floats for all 2049 bins of n_fft 4096
    p->dev.band_lo = band_lo_bin;
    p->dev.nband = band_hi_bin - band_lo_bin + 1;
    p->band_ok = band_lo_bin >= 0 && band_hi_bin <= N / 2 && p->dev.nband >= 1;
    p->dev.stride = p->band_ok ? (p->dev.nband + 63) & ~63 : kFS;
    p->w2h = w2;
    p->envh = env;
    *out = p.release();
    return AWARE_OK;
}

extern "C" int aware_plan_create(aware_plan** out, int n_fft, int hop, int win_length, int window, int band_lo_bin,
                                 int band_hi_bin) {
    return aware_plan_create_ex(out, n_fft, hop, win_length, window, band_lo_bin, band_hi_bin, 0);
}

extern "C" int aware_plan_create_ex(aware_plan** out, int n_fft, int hop, int win_length, int window, int band_lo_bin,
                                    int band_hi_bin, int flags) {
    if (!out || (flags & ~AWARE_PLAN_GENERAL)) return AWARE_E_BADARG;
    if (n_fft != kNfft || hop != kHop || win_length != kNfft || (flags & AWARE_PLAN_GENERAL))
        return gen_plan_create(out, n_fft, hop, win_length, window, band_lo_bin, band_hi_bin, flags);
    if (window != 0 && window != 1) return AWARE_E_BADARG;
    const int nband = band_hi_bin - band_lo_bin + 1;
    // any band of the one-sided spectrum: narrow layout (kFS columns) inside bins 1..511 up to 256 bins wide, else wide
    if (band_lo_bin < 0 || band_hi_bin > kNfft / 2 || nband < 1) return AWARE_E_UNSUPPORTED;
    const double PI = 3.14159265358979323846;
    std::vector<float> h(2 * 512 + 2 * 512 + 1024 + 1024 + 3 * 768);
    float* tw512 = h.data();
    float* tw1024 = tw512 + 1024;
    float* win = tw1024 + 1024;
    float* win2 = win + 1024;
    for (int j = 0; j < 512; ++j) {
        tw512[2 * j] = (float)cos(2 * PI * j / 512);
        tw512[2 * j + 1] = (float)-sin(2 * PI * j / 512);
        tw1024[2 * j] = (float)cos(2 * PI * j / 1024);
        tw1024[2 * j + 1] = (float)-sin(2 * PI * j / 1024);
    }
    for (int i = 0; i < 1024; ++i) {
        // torch.hann_window / torch.hamming_window (periodic), utils/audio/stft.py:19-25
        double w = (window == 0) ? 0.5 - 0.5 * cos(2 * PI * i / 1024) : 0.54 - 0.46 * cos(2 * PI * i / 1024);
        win[i] = (float)w;
        win2[i] = win[i] * win[i];
    }
    // overlap-add envelope tables, summed in ascending frame order like ola_envelope_loop
    float* env = win2 + 1024;
    for (int q = 0; q < 768; ++q) {
        float e = 0.f;
        for (int t = 0; t <= (q >> 8); ++t) e += win2[q - 256 * t];
        env[q] = e;                                               // head: p = q < 768
        float ei = 0.f;
        for (int off = (q & 255) + 768; off >= (q & 255); off -= 256) ei += win2[off];
        env[768 + q] = ei;                                        // interior: p mod 256 = q & 255
        float et = 0.f;
        for (int off = (q & 255) + 768; off >= q + 256; off -= 256) et += win2[off];
        env[1536 + q] = et;                                       // tail: p = 256*T + q
    }
    Building<aware_plan, aware_plan_destroy> p(new aware_plan());
    HIPCHK(hipMalloc(&p->mem, h.size() * sizeof(float)));
    HIPCHK(hipMemcpy(p->mem, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    float* d = (float*)p->mem;
    p->dev.tw512 = (const cf*)d;
    p->dev.tw1024 = (const cf*)(d + 1024);
    p->dev.window = d + 2048;
    p->dev.window2 = d + 3072;
    p->dev.env_tab = d + 4096;
    p->dev.band_lo = band_lo_bin;
    p->dev.nband = nband;
    p->dev.stride = band_stride_for(band_lo_bin, band_hi_bin);
    *out = p.release();
    return AWARE_OK;
}
extern "C" void aware_plan_destroy(aware_plan* p) {
    if (!p) return;
    if (p->mem) (void)hipFree(p->mem);
    delete p;
}
extern "C" int aware_plan_spectrum_stride(const aware_plan* p) {
    return p ? (p->general ? p->gdev.stride : AWARE_FULL_STRIDE) : AWARE_E_BADARG;
}
extern "C" int aware_plan_is_general(const aware_plan* p) { return p ? p->general : AWARE_E_BADARG; }
extern "C" int aware_plan_band_stride(const aware_plan* p) { return p ? p->dev.stride : AWARE_E_BADARG; }

extern "C" int aware_nola_check(int n_fft, int hop, int win_length, int window, int n_samples) {
    const int rc = gen_validate(n_fft, hop, win_length, window);
    if (rc != AWARE_OK) return rc;
    if (n_samples < 0) return AWARE_E_BADARG;
    std::vector<float> w, w2, env;
    gen_host_tables(n_fft, hop, win_length, window, w, w2, env);
    return gen_nola_ok(env.data(), w2.data(), n_fft, hop, 1 + n_samples / hop) ? AWARE_OK : AWARE_E_BADARG;
}

// ---------------------------------------------------------------------------------------------
// The host tables of a batch into its one device allocation d_mem, one behind the other: those of both routes, then the
// route's own.  An empty table is not copied and keeps a null pointer.  Returns the first error.
static hipError_t upload_tables(aware_batch* b, std::initializer_list<std::pair<int**, const std::vector<int>*>> own) {
    int* d = b->d_mem;
    hipError_t e = hipSuccess;
    auto up = [&](int*& dst, const std::vector<int>& v) {
        if (e != hipSuccess || v.empty()) return;
        dst = d; d += v.size();
        e = hipMemcpy(dst, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice);
    };
    up(b->d_frame_off, b->frame_off); up(b->d_pool_off, b->pool_off); up(b->d_in_off, b->in_off); up(b->d_in_len, b->n);
    up(b->d_out_off, b->out_off); up(b->d_out_len, b->out_len); up(b->d_pc_in, b->pc_in); up(b->d_order, b->order);
    for (const auto& t : own) up(*t.first, *t.second);
    return e;
}
extern "C" int aware_batch_create(aware_batch** out, int B, const int* n_samples, const int* in_offsets) {
    if (!out || B < 1 || !n_samples) return AWARE_E_BADARG;
    Building<aware_batch, aware_batch_destroy> b(new aware_batch());
    b->B = B;
    b->n.assign(n_samples, n_samples + B);
    // torch.stft's reflect padding needs n > n_fft/2
    if (!batch_layout(n_samples, in_offsets, B, kHop, kHalf, *b)) return AWARE_E_BADARG;
    card_runs(n_samples, kHop, kStreamWaves, kSynthBlocks, *b, *b);
    const size_t ints = (size_t)(B + 1) * 2 + (size_t)B * 7 + b->an_wg.size() + b->syn_wg.size();
    HIPCHK(hipMalloc((void**)&b->d_mem, ints * sizeof(int)));
    HIPCHK(upload_tables(b.get(), {{&b->d_pc_syn, &b->pc_syn}, {&b->d_an_wg, &b->an_wg}, {&b->d_syn_wg, &b->syn_wg}}));
    *out = b.release();
    return AWARE_OK;
}
static int gen_batch_create(aware_batch** out, const aware_plan* plan, int B, const int* n_samples, const int* in_offsets) {
    const int N = plan->n_fft, hop = plan->hop;
    Building<aware_batch, aware_batch_destroy> b(new aware_batch());
    b->general = 1;
    b->g_nfft = N; b->g_hop = hop; b->g_win = plan->win_length; b->g_window = plan->window;
    b->B = B;
    b->n.assign(n_samples, n_samples + B);
    if (!batch_layout(n_samples, in_offsets, B, hop, N / 2, *b)) return AWARE_E_BADARG;      // n > n_fft/2, as on the card route
    b->synth_run = kSynthBlocks;      // no runs on this route: aware_batch_synth_run reports the staged kernels' block count
    const std::vector<int> pc_out = pc_out_for(b->out_len);
    for (int i = 0; i < B; ++i) b->nola_ok = b->nola_ok && gen_nola_ok(plan->envh.data(), plan->w2h.data(), N, hop, b->T[i]);
    const size_t ints = (size_t)(B + 1) * 2 + (size_t)B * 7;
    if (hipMalloc((void**)&b->d_mem, ints * sizeof(int)) != hipSuccess ||
        hipMalloc((void**)&b->d_frames, (size_t)b->NF * N * sizeof(float)) != hipSuccess) {
        g_last_err = "aware_batch_create_for_plan: device memory";
        return AWARE_E_HIP;
    }
    const hipError_t e = upload_tables(b.get(), {{&b->d_pc_out, &pc_out}});
    if (e != hipSuccess) {
        g_last_err = std::string("aware_batch_create_for_plan: ") + hipGetErrorString(e);
        return AWARE_E_HIP;
    }
    *out = b.release();
    return AWARE_OK;
}

extern "C" int aware_batch_create_for_plan(aware_batch** out, const aware_plan* plan, int B, const int* n_samples,
                                           const int* in_offsets) {
    if (!out || !plan || B < 1 || !n_samples) return AWARE_E_BADARG;
    if (!plan->general) return aware_batch_create(out, B, n_samples, in_offsets);
    return gen_batch_create(out, plan, B, n_samples, in_offsets);
}

extern "C" void aware_batch_destroy(aware_batch* b) {
    if (!b) return;
    if (b->d_mem) (void)hipFree(b->d_mem);
    if (b->d_frames) (void)hipFree(b->d_frames);
    delete b;
}
extern "C" int aware_batch_total_frames(const aware_batch* b) { return b ? b->NF : AWARE_E_BADARG; }
extern "C" int aware_batch_total_pooled(const aware_batch* b) { return b ? b->NP : AWARE_E_BADARG; }
extern "C" int aware_batch_total_out(const aware_batch* b) { return b ? b->NS : AWARE_E_BADARG; }
extern "C" int aware_batch_synth_run(const aware_batch* b) { return b ? b->synth_run : AWARE_E_BADARG; }
extern "C" int aware_batch_analysis_run(const aware_batch* b) { return b ? b->an_run : AWARE_E_BADARG; }
extern "C" int aware_batch_out_offset(const aware_batch* b, int i) {
    return (b && i >= 0 && i < b->B) ? b->out_off[i] : AWARE_E_BADARG;
}
extern "C" int aware_batch_out_length(const aware_batch* b, int i) {
    return (b && i >= 0 && i < b->B) ? b->out_len[i] : AWARE_E_BADARG;
}
extern "C" int aware_batch_frames(const aware_batch* b, int i) {
    return (b && i >= 0 && i < b->B) ? b->T[i] : AWARE_E_BADARG;
}
extern "C" size_t aware_batch_scratch_bytes(const aware_batch* b) {
    return b ? (size_t)b->B * b->pstride * sizeof(unsigned long long) + 256 : 0;
}

// ---- general-geometry dispatch (stft_any.hip) ----
static bool gen_batch_matches(const aware_plan* plan, const aware_batch* b) {
    return b->general && b->g_nfft == plan->n_fft && b->g_hop == plan->hop && b->g_win == plan->win_length &&
           b->g_window == plan->window;
}
static GenLaunch gen_launch(const aware_plan* plan, const aware_batch* b) {
    GenLaunch L;
    L.plan = plan->gdev;
    L.B = b->B; L.NF = b->NF; L.max_len = b->max_len;
    L.frame_off = b->d_frame_off;
    L.sig_off = b->d_in_off; L.sig_len = b->d_in_len;
    L.out_off = b->d_out_off; L.out_len = b->d_out_len;
    L.pstride = b->pstride;
    L.frames = b->d_frames;
    return L;
}
// ---- card dispatch (dsp_kernels.hip, dsp_stream.hip): what every launch of a transform takes from its plan and its batch;
// everything else is set where the launch is made.  The analysis reads `sig` on the caller's layout (clip i at in_off[i], n_i
// samples, one partial maximum per 4096 of them), or on the loop's (at out_off[i], hop (T_i - 1) samples, one per synthesis run)
static AnalysisLaunch analysis_launch(const aware_plan* plan, const aware_batch* b, const float* sig, bool loop_layout) {
    AnalysisLaunch L;
    L.plan = plan->dev; L.frame_off = b->d_frame_off; L.B = b->B; L.max_frames = b->max_frames;
    L.run_frames = b->an_run; L.wg_tab = b->d_an_wg; L.n_wg = (int)b->an_wg.size();
    L.sig = sig; L.sig_off = loop_layout ? b->d_out_off : b->d_in_off; L.sig_len = loop_layout ? b->d_out_len : b->d_in_len;
    L.pcount = loop_layout ? b->d_pc_syn : b->d_pc_in; L.pstride = b->pstride;
    return L;
}
static SynthLaunch synth_launch(const aware_plan* plan, const aware_batch* b) {
    SynthLaunch S;
    S.plan = plan->dev; S.frame_off = b->d_frame_off; S.B = b->B; S.max_frames = b->max_frames;
    S.run_blocks = b->synth_run; S.wg_tab = b->d_syn_wg; S.n_wg = (int)b->syn_wg.size();
    return S;
}
static int gen_stft(const aware_plan* plan, const aware_batch* b, const float* audio, int normalize, void* spec,
                    void* scratch, hipStream_t st) {
    if (!gen_batch_matches(plan, b)) return AWARE_E_BADARG;
    GenLaunch L = gen_launch(plan, b);
    if (normalize) {
        unsigned long long* pmax = (unsigned long long*)scratch;
        launch_absmax_partials(audio, b->d_in_off, b->d_in_len, pmax, b->pstride, b->B, b->max_len, st);
        LAUNCHCHK();
        L.pmax = pmax; L.pcount = b->d_pc_in;
    }
    launch_gen_analysis(L, audio, spec, 0, st);
    LAUNCHCHK();
    return AWARE_OK;
}
static int gen_istft(const aware_plan* plan, const aware_batch* b, const void* spec, int normalize, float* out,
                     void* scratch, hipStream_t st) {
    if (!gen_batch_matches(plan, b) || !b->nola_ok) return AWARE_E_BADARG;
    GenLaunch L = gen_launch(plan, b);
    launch_gen_synthesis(L, spec, out, 0, st);
    LAUNCHCHK();
    if (normalize) {
        unsigned long long* pmax = (unsigned long long*)scratch;
        launch_absmax_partials(out, b->d_out_off, b->d_out_len, pmax, b->pstride, b->B, b->max_len, st);
        LAUNCHCHK();
        L.pmax = pmax; L.pcount = b->d_pc_out;
        launch_gen_normalize(L, out, st);
        LAUNCHCHK();
    }
    return AWARE_OK;
}

// The DSP kernels exist in two forms: streaming wave kernels (dsp_stream.hip; default wherever the band lies inside bins
// 1..256) and workgroup-staged kernels (dsp_kernels.hip; any band, full-spectrum input/output, and the form the
// streaming kernels are tested against).  dsp_path: 0 = streaming where supported, 1 = staged.
static void run_analysis(AnalysisLaunch& L, int dsp_path, hipStream_t st) {
    if (dsp_path == 0 && !L.full && stream_supported(L.plan)) { L.stream = 1; launch_analysis_stream(L, st); }
    else launch_analysis(L, st);
}
static void run_synth(SynthLaunch& S, int dsp_path, hipStream_t st) {
    if (dsp_path == 0 && !S.full && stream_supported(S.plan)) { S.stream = 1; launch_synth_stream(S, st); }
    else launch_synth(S, st);
}

// ---------------------------------------------------------------------------------------------
// workspace carving: Carver is in loop_chain.hpp

// ---------------------------------------------------------------------------------------------
extern "C" int aware_stft(const aware_plan* plan, const aware_batch* b, const float* audio, int normalize, void* spec,
                          void* scratch, void* stream) {
    if (!plan || !b || !audio || !spec || (normalize && !scratch)) return AWARE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (plan->general) return gen_stft(plan, b, audio, normalize, spec, scratch, st);
    if (b->general) return AWARE_E_BADARG;
    unsigned long long* pmax = (unsigned long long*)scratch;
    if (normalize) {
        launch_absmax_partials(audio, b->d_in_off, b->d_in_len, pmax, b->pstride, b->B, b->max_len, st);
        LAUNCHCHK();
    }
    AnalysisLaunch L = analysis_launch(plan, b, audio, false);
    L.pmax = normalize ? pmax : nullptr;
    L.full = spec;
    launch_analysis(L, st);
    LAUNCHCHK();
    return AWARE_OK;
}

extern "C" int aware_stft_band(const aware_plan* plan, const aware_batch* b, const float* audio, int normalize,
                               float* mag, void* phasor, void* scratch, void* stream) {
    if (!plan || !b || !audio || (!mag && !phasor) || (normalize && !scratch)) return AWARE_E_BADARG;
    if (plan->general) return AWARE_E_UNSUPPORTED;
    if (b->general) return AWARE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* pmax = (unsigned long long*)scratch;
    if (normalize) {
        launch_absmax_partials(audio, b->d_in_off, b->d_in_len, pmax, b->pstride, b->B, b->max_len, st);
        LAUNCHCHK();
    }
    AnalysisLaunch L = analysis_launch(plan, b, audio, false);
    L.pmax = normalize ? pmax : nullptr;
    L.mag = mag; L.unit = phasor; L.unit_default = 1.f;
    L.polar_exact = 1;       // the original audio: the decomposer's magnitudes and phasors, and the magnitudes detection reads
    run_analysis(L, 0, st);
    LAUNCHCHK();
    return AWARE_OK;
}

extern "C" int aware_istft(const aware_plan* plan, const aware_batch* b, const void* spec, int normalize, float* out,
                           void* scratch, void* stream) {
    if (!plan || !b || !spec || !out || (normalize && !scratch)) return AWARE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (plan->general) return gen_istft(plan, b, spec, normalize, out, scratch, st);
    if (b->general) return AWARE_E_BADARG;
    unsigned long long* pmax = (unsigned long long*)scratch;
    SynthLaunch S = synth_launch(plan, b);
    S.full = spec; S.out = out; S.pmax = normalize ? pmax : nullptr; S.pstride = b->pstride;
    launch_synth(S, st);
    LAUNCHCHK();
    if (normalize) {
        launch_finish(out, b->d_frame_off, pmax, b->d_pc_syn, b->pstride, nullptr, out, b->d_out_off, b->B,
                      b->max_frames, st);
        LAUNCHCHK();
    }
    return AWARE_OK;
}

// ---- backward of the two transforms for the differentiable plug-in seam (interfaces/audio.py:6-9) ----
extern "C" int aware_stft_bwd(const aware_plan* plan, const aware_batch* b, const void* grad_spec, float* grad_audio,
                              void* stream) {
    if (!plan || !b || !grad_spec || !grad_audio) return AWARE_E_BADARG;
    if (plan->general) {
        if (!gen_batch_matches(plan, b)) return AWARE_E_BADARG;
        launch_gen_synthesis(gen_launch(plan, b), grad_spec, grad_audio, 1, (hipStream_t)stream);
        LAUNCHCHK();
        return AWARE_OK;
    }
    if (b->general) return AWARE_E_BADARG;
    // the staged synthesis kernel in adjoint mode: overlap-add of the windowed rfft adjoints, then the fold of the two reflect
    // pads for a clip of any length n > 512 at the clip's offset in the caller's ragged array
    for (int i = 0; i < b->B; ++i)
        if (run_cuts_short_segments(b->T[i] - 1, b->synth_run)) return AWARE_E_UNSUPPORTED;      // (synth_run_for never picks such a run)
    SynthLaunch S = synth_launch(plan, b);
    S.full = grad_spec; S.out = grad_audio; S.adjoint = 1; S.pstride = b->pstride;
    S.sig_off = b->d_in_off; S.sig_len = b->d_in_len;
    launch_synth(S, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

extern "C" int aware_istft_bwd(const aware_plan* plan, const aware_batch* b, const float* grad_audio, void* grad_spec,
                               void* stream) {
    if (!plan || !b || !grad_audio || !grad_spec) return AWARE_E_BADARG;
    if (plan->general) {
        if (!gen_batch_matches(plan, b) || !b->nola_ok) return AWARE_E_BADARG;
        launch_gen_analysis(gen_launch(plan, b), grad_audio, grad_spec, 1, (hipStream_t)stream);
        LAUNCHCHK();
        return AWARE_OK;
    }
    if (b->general) return AWARE_E_BADARG;
    AnalysisLaunch L = analysis_launch(plan, b, grad_audio, true);
    L.full = grad_spec; L.adjoint = 1;
    launch_analysis(L, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

// ---------------------------------------------------------------------------------------------
extern "C" void aware_detector_destroy(aware_detector* d);
// whether the training extension serves the detector: the model card's architecture on 128 mel bands, hidden widths stored
// as given and at most 7 layers (it adds no padding logic of its own)
static bool det_trainable(const aware_detector* d) {
    if (!d->card_arch || d->n_mels != 128 || d->n_layers > 7) return false;
    for (int i = 0; i < d->n_layers; ++i)
        if (d->ch[i] != d->uch[i]) return false;
    return true;
}
// detector_image.hpp does the host arithmetic of a detector's parameters; here are its arguments and the device calls
static const DetectorLimits kDetLimits{kMaxTapKernel, kMaxTapStride, kMinPool, kMaxPool};
static const MelTapShape kMelShape{kFS, kMelTapsA, kMelTapsB};
static const PackRules kPackRules{x3_packed_bytes, h2_packed_bytes, gemm_clip_h2_supported, readout_x3_supported};
// a host image into its device buffer, which is `room` bytes and allocated here where `alloc`
static int det_put(void** mem, bool alloc, size_t room, const void* src, size_t bytes) {
    if (alloc) HIPCHK(hipMalloc(mem, room));
    HIPCHK(hipMemcpy(*mem, src, bytes, hipMemcpyHostToDevice));
    return AWARE_OK;
}
static void* det_at(void* mem, const PackSlot& t) { return t.on ? (char*)mem + t.off : nullptr; }
// the two sparse mel forms, one buffer: tw, fw, tm, fs (allocated the first time a basis has the two-tap form)
static int upload_mel_forms(aware_detector* d, const MelForms& m) {
    d->melw = nullptr; d->melm = nullptr; d->melf_w = nullptr; d->melf_s = nullptr;
    if (!m.sparse) return AWARE_OK;
    const size_t b_tw = m.tw.size() * sizeof(float), b_fw = m.fw.size() * sizeof(float);
    if (!d->mel2mem) HIPCHK(hipMalloc(&d->mel2mem, b_tw + b_fw + m.tm.size() + m.fs.size() + 64));
    char* base = (char*)d->mel2mem;
    unsigned char* bytes = (unsigned char*)base + b_tw + b_fw;
    HIPCHK(hipMemcpy(base, m.tw.data(), b_tw, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(bytes, m.tm.data(), m.tm.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(base + b_tw, m.fw.data(), b_fw, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(bytes + m.tm.size(), m.fs.data(), m.fs.size(), hipMemcpyHostToDevice));
    d->melw = (float2*)base;
    d->melm = bytes;
    if (m.runs) { d->melf_w = (float*)(base + b_tw); d->melf_s = bytes + m.tm.size(); }
    return AWARE_OK;
}
// the bf16x3 fragment images, packed on the host
static int upload_x3(aware_detector* d, const DetectorImage& im, const PackedLayout& L, bool alloc) {
    std::vector<uint16_t> hp(L.x3_total / 2 + 8, 0);
    auto pack = [&](const PackSlot& t, const float* src) { if (t.on) x3_pack(src, t.N, t.K, hp.data() + t.off / 2); };
    pack(L.last, L.last_rows.data());
    pack(L.lastT, L.lastT_rows.data());
    pack(L.melT, im.h.data() + im.o_melT);
    pack(L.melB, im.h.data() + im.o_melB);
    for (int l = 0; l < d->n_layers; ++l) {
        pack(L.w[l], im.h.data() + im.o_w[l]);
        pack(L.wT[l], im.h.data() + im.o_wT[l]);
    }
    const int rc = det_put(&d->pkmem, alloc, L.x3_total + 16, hp.data(), L.x3_total);
    if (rc) return rc;
    d->lastpk = det_at(d->pkmem, L.last); d->lastTpk = det_at(d->pkmem, L.lastT);
    d->melTpk = det_at(d->pkmem, L.melT); d->melBpk = det_at(d->pkmem, L.melB);
    for (int l = 0; l < d->n_layers; ++l) { d->wpk[l] = det_at(d->pkmem, L.w[l]); d->wTpk[l] = det_at(d->pkmem, L.wT[l]); }
    return AWARE_OK;
}
// the f16 two-term images, packed on the device from the f32 copies just uploaded
static int upload_h2(aware_detector* d, const PackedLayout& L, bool alloc) {
    if (!L.h2_total) return AWARE_OK;
    if (alloc) HIPCHK(hipMalloc(&d->h2mem, L.h2_total));
    for (int l = 0; l < d->n_layers; ++l) {
        d->wh2[l] = det_at(d->h2mem, L.wh2[l]); d->wTh2[l] = det_at(d->h2mem, L.wTh2[l]);
        if (d->wh2[l]) launch_h2_pack(d->w[l], L.wh2[l].K, L.wh2[l].N, L.wh2[l].K, d->wh2[l], 0);
        if (d->wTh2[l]) launch_h2_pack(d->wT[l], L.wTh2[l].K, L.wTh2[l].N, L.wTh2[l].K, d->wTh2[l], 0);
    }
    LAUNCHCHK();
    HIPCHK(hipStreamSynchronize(0));
    return AWARE_OK;
}
// host staging of the detector's parameters (plain + transposed f32 copies, bf16x3 fragment images) and upload; `alloc`
// = false re-uses the device buffers of a detector created with the same shapes (aware_detector_update)
static int detector_upload(aware_detector* d, const DetectorSpec& s, const float* mel_basis, const float* const* weights,
                           const float* const* biases, bool alloc) {
    const DetectorBand band{d->band_lo, d->nband, d->stride, d->n_fft, d->general};
    const DetectorImage im = detector_image(s, band, mel_basis, weights, biases);
    int rc = upload_mel_forms(d, mel_forms(s, band, im, kMelShape));
    if (rc) return rc;
    const size_t bytes = im.h.size() * sizeof(float);
    if ((rc = det_put((void**)&d->mem, alloc, bytes, im.h.data(), bytes))) return rc;
    d->melT = d->mem + im.o_melT;
    d->melB = d->mem + im.o_melB;
    for (int l = 0; l < d->n_layers; ++l) { d->w[l] = d->mem + im.o_w[l]; d->wT[l] = d->mem + im.o_wT[l]; d->bias[l] = d->mem + im.o_b[l]; }
    const PackedLayout L = packed_layout(s, band, im, kPackRules);
    if ((rc = upload_x3(d, im, L, alloc))) return rc;
    return upload_h2(d, L, alloc);
}
// the folded BatchNorm map of every block
static int upload_norm(aware_detector* d, const NormImage& n) {
    const size_t bytes = n.h.size() * sizeof(float);
    const int rc = det_put((void**)&d->normmem, true, bytes, n.h.data(), bytes);
    if (rc) return rc;
    for (int l = 0; l < d->n_layers; ++l) { d->nscale[l] = d->normmem + n.o_scale[l]; d->nshift[l] = d->normmem + n.o_shift[l]; }
    return AWARE_OK;
}

// the one create path: every aware_detector_create* fills a spec (detector_image.hpp: DetectorSpec) and comes here
static int detector_create(aware_detector** out, const aware_plan* plan, const float* mel_basis, const DetectorSpec& s,
                           const float* const* weights, const float* const* biases) {
    // plan_ok: not a general plan made for the transforms alone (no AWARE_PLAN_GENERAL), or with a band outside bins 0..n_fft/2
    int rc = detector_spec_check(s, kDetLimits, out && plan && mel_basis && weights,
                                 !plan || !plan->general || (plan->loop && plan->band_ok));
    if (rc) return rc;
    const int n_layers = s.n_layers;
    Building<aware_detector, aware_detector_destroy> d(new aware_detector());
    d->n_mels = s.n_mels; d->n_layers = n_layers; d->nbits = s.channels[n_layers] / 2;
    d->band_lo = plan->dev.band_lo; d->nband = plan->dev.nband; d->stride = plan->dev.stride;
    d->n_fft = plan->n_fft; d->general = plan->general != 0;
    d->uch.assign(s.channels, s.channels + n_layers + 1);
    for (int i = 0; i <= n_layers; ++i) {
        d->ch.push_back(s.stored(i));
        d->maxc = std::max(d->maxc, d->ch[i]);
        if (i < n_layers) d->max_cin = std::max(d->max_cin, d->ch[i]);
    }
    d->taps = s.taps();
    d->tk = s.kernel_size; d->ts = s.stride; d->tp = s.padding;
    d->pooled = s.pooled();
    d->psize = s.pool_size; d->pstride = s.pool_stride;
    d->w.assign(n_layers, nullptr); d->wT.assign(n_layers, nullptr); d->bias.assign(n_layers, nullptr);
    d->wpk.assign(n_layers, nullptr); d->wTpk.assign(n_layers, nullptr);
    d->wh2.assign(n_layers, nullptr); d->wTh2.assign(n_layers, nullptr);
    d->nscale.assign(n_layers, nullptr); d->nshift.assign(n_layers, nullptr);
    if (s.arch) {
        d->act = s.arch->activation; d->norm = s.arch->norm; d->final_act = s.arch->final_activation;
        d->card_arch = d->act == kActLRelu && d->norm == kNormInstance && d->final_act == kActTanh;
    }
    if (d->taps || d->pooled) d->card_arch = false;
    rc = detector_upload(d.get(), s, mel_basis, weights, biases, true);
    if (rc == AWARE_OK && d->norm == kNormAffine) rc = upload_norm(d.get(), norm_image(s));
    if (rc) return rc;
    *out = d.release();
    return AWARE_OK;
}
extern "C" int aware_detector_create(aware_detector** out, const aware_plan* plan, const float* mel_basis, int n_mels,
                                     int n_layers, const int* channels, const float* const* weights,
                                     const float* const* biases) {
    return detector_create(out, plan, mel_basis, DetectorSpec{n_mels, n_layers, channels}, weights, biases);
}
extern "C" int aware_detector_create_ex(aware_detector** out, const aware_plan* plan, const float* mel_basis, int n_mels,
                                        int n_layers, const int* channels, const float* const* weights,
                                        const float* const* biases, const aware_detector_arch* arch) {
    return detector_create(out, plan, mel_basis, DetectorSpec{n_mels, n_layers, channels, arch, true}, weights, biases);
}
// The same for a detector of temporal convolutions: every block Conv1d(C_in, C_out, kernel_size, stride, padding) along the
// pooled frames (conv_taps.hpp); weights[l] is [Cout][Cin][kernel_size].  1 / 1 / 0 is aware_detector_create_ex.
extern "C" int aware_detector_create_conv(aware_detector** out, const aware_plan* plan, const float* mel_basis, int n_mels,
                                          int n_layers, const int* channels, const float* const* weights,
                                          const float* const* biases, const aware_detector_arch* arch, int kernel_size, int stride,
                                          int padding) {
    return detector_create(out, plan, mel_basis, DetectorSpec{n_mels, n_layers, channels, arch, true, kernel_size, stride, padding},
                           weights, biases);
}
// The same with the initial pool AvgPool1d(pool_size, pool_stride) between the mel stage and block 0 (conv_taps.hpp: pool_rows).
// 2 / 2 is aware_detector_create_conv.
extern "C" int aware_detector_create_pool(aware_detector** out, const aware_plan* plan, const float* mel_basis, int n_mels,
                                          int n_layers, const int* channels, const float* const* weights,
                                          const float* const* biases, const aware_detector_arch* arch, int kernel_size, int stride,
                                          int padding, int pool_size, int pool_stride) {
    return detector_create(out, plan, mel_basis, DetectorSpec{n_mels, n_layers, channels, arch, true, kernel_size, stride, padding,
                                                              pool_size, pool_stride}, weights, biases);
}
extern "C" int aware_detector_pool(const aware_detector* d, int* pool_size, int* pool_stride) {
    if (!d) return AWARE_E_BADARG;
    if (pool_size) *pool_size = d->psize;
    if (pool_stride) *pool_stride = d->pstride;
    return AWARE_OK;
}
extern "C" int aware_pool_rows(int frames, int pool_size, int pool_stride) {
    if (frames < 0 || pool_size < 1 || pool_stride < 1) return AWARE_E_BADARG;
    return pool_rows(frames, pool_size, pool_stride);
}
extern "C" int aware_detector_conv(const aware_detector* d, int* kernel_size, int* stride, int* padding) {
    if (!d) return AWARE_E_BADARG;
    if (kernel_size) *kernel_size = d->tk;
    if (stride) *stride = d->ts;
    if (padding) *padding = d->tp;
    return AWARE_OK;
}
// The row rule and the two data-movement kernels of the temporal convolutions on their own (conv_taps.hpp), for callers that
// check them: x / dx [total pooled rows][channels], u / du [total pooled rows][kernel_size * channels], channels % 4 == 0
extern "C" int aware_conv_rows(int rows, int blocks, int kernel_size, int stride, int padding) {
    if (rows < 0 || blocks < 0 || kernel_size < 1 || stride < 1 || padding < 0) return AWARE_E_BADARG;
    return conv_rows(rows, blocks, kernel_size, stride, padding);
}
static int conv_taps_args(const aware_batch* b, const void* in, const void* out, int channels, int block, int k, int s, int p) {
    if (!b || !in || !out || channels < 4 || channels % 4 || block < 0 || block >= kMaxLayers) return AWARE_E_BADARG;
    if (k < 1 || s < 1 || p < 0) return AWARE_E_BADARG;
    if (k > kMaxTapKernel || s > kMaxTapStride || 2 * p > k - 1) return AWARE_E_UNSUPPORTED;
    return AWARE_OK;
}
extern "C" int aware_conv_unfold(const aware_batch* b, const float* x, float* u, int channels, int block, int kernel_size,
                                 int stride, int padding, void* stream) {
    const int rc = conv_taps_args(b, x, u, channels, block, kernel_size, stride, padding);
    if (rc) return rc;
    launch_conv_unfold(x, u, b->d_frame_off, b->d_pool_off, channels, b->B, b->max_frames / 2, block, kernel_size, stride, padding,
                       (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}
extern "C" int aware_conv_fold(const aware_batch* b, const float* du, float* dx, int channels, int block, int kernel_size,
                               int stride, int padding, void* stream) {
    const int rc = conv_taps_args(b, du, dx, channels, block, kernel_size, stride, padding);
    if (rc) return rc;
    launch_conv_fold(du, dx, b->d_frame_off, b->d_pool_off, channels, b->B, b->max_frames / 2, block, kernel_size, stride, padding,
                     (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}
extern "C" int aware_detector_is_card(const aware_detector* d) { return d ? (d->card_arch ? 1 : 0) : AWARE_E_BADARG; }
// EXTENSION (detector training, BASELINE north_star; the reference never changes the weights): replace the parameters of a
// detector in place (same layer shapes).  Host arrays as for aware_detector_create.  Synchronous (blocking copies); the
// caller makes sure no work using the detector is in flight.
extern "C" int aware_detector_update(aware_detector* d, const float* mel_basis, const float* const* weights,
                                     const float* const* biases) {
    if (!d || !mel_basis || !weights) return AWARE_E_BADARG;
    if (!det_trainable(d)) return AWARE_E_UNSUPPORTED;   // the training extension serves the model card's network only
    const DetectorSpec s{d->n_mels, d->n_layers, d->uch.data()};   // (a trainable detector has 1x1 blocks and the (2, 2) pool)
    return detector_upload(d, s, mel_basis, weights, biases, false);
}
// EXTENSION (detector training): the same refresh from DEVICE arrays, asynchronous on `stream` -- no host round trip of the
// 1.68 M parameters: copies, transposes, bf16 three-term and f16 two-term images all rebuilt by kernels.  dev_weights[l]:
// [Cout][Cin] f32, dev_biases[l]: [Cout] f32 (device pointers in host arrays; biases may be NULL = unchanged).
extern "C" int aware_detector_update_device(aware_detector* d, const float* const* dev_weights, const float* const* dev_biases,
                                            void* stream) {
    if (!d || !dev_weights) return AWARE_E_BADARG;
    if (!det_trainable(d)) return AWARE_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const int nl = d->n_layers;
    for (int l = 0; l < nl; ++l) {
        const int ci = d->ch[l], co = d->ch[l + 1];
        const int rows = l == nl - 1 ? 2 * d->nbits : co;   // the caller's rows; the padding rows stay zero
        if (!dev_weights[l]) return AWARE_E_BADARG;
        HIPCHK(hipMemcpyAsync(d->w[l], dev_weights[l], (size_t)ci * rows * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (dev_biases && dev_biases[l])
            HIPCHK(hipMemcpyAsync(d->bias[l], dev_biases[l], (size_t)rows * sizeof(float), hipMemcpyDeviceToDevice, st));
        launch_transpose(d->w[l], d->wT[l], co, ci, st);
        if (d->wpk[l]) launch_x3_pack_dev(d->w[l], ci, co, ci, co, ci, d->wpk[l], st);
        if (d->wTpk[l]) launch_x3_pack_dev(d->wT[l], co, ci, co, ci, co, d->wTpk[l], st);
        if (d->wh2[l]) launch_h2_pack(d->w[l], ci, co, ci, d->wh2[l], st);
        if (d->wTh2[l]) launch_h2_pack(d->wT[l], co, ci, co, d->wTh2[l], st);
    }
    if (d->lastpk) {
        const int cil = d->ch[nl - 1], col = d->ch[nl], colp = 16 * ((col + 15) / 16);
        launch_x3_pack_dev(d->w[nl - 1], cil, col, cil, colp, cil, d->lastpk, st);        // rows zero-padded to a multiple of 16
        launch_x3_pack_dev(d->wT[nl - 1], col, cil, col, cil, 64, d->lastTpk, st);        // k zero-padded to 64
    }
    LAUNCHCHK();
    return AWARE_OK;
}

extern "C" void aware_detector_destroy(aware_detector* d) {
    if (!d) return;
    if (d->mem) (void)hipFree(d->mem);
    if (d->pkmem) (void)hipFree(d->pkmem);
    if (d->h2mem) (void)hipFree(d->h2mem);
    if (d->mel2mem) (void)hipFree(d->mel2mem);
    if (d->normmem) (void)hipFree(d->normmem);
    delete d;
}

// Plain GEMM C[M][N] = A[M][K] * Bt^T on the bf16x3 kernel when its packed operand exists and the shape fits
// (32-row blocks play the role of clips; plain epilogue), else on the f32-MFMA kernel.
static void gemm_plain(int pipe, const float* A, int lda, const float* Bt, int ldb, const void* Bpk, const float* bias, float* C,
                       int ldc, int M, int N, int K, hipStream_t st) {
    if (pipe != 1 && Bpk && gemm_clip_x3_supported(1, N, K, lda)) {
        // tile height: a workgroup streams its whole weight slab (6 K N/tn bytes) for its rows, so taller tiles cut the L2
        // traffic of these short-K GEMMs; keep at least two workgroups per CU's worth of tiles.  M need not be a multiple
        // of the tile height (ragged batches): the last row block is partial
        const long blocks32 = (M + 31) / 32;
        const int g = (blocks32 * (N / 128) / 2 >= 512) ? 2 : 1;
        const int nb = (int)((M + 32 * g - 1) / (32 * g));
        launch_gemm_clip_x3(A, lda, Bpk, bias, C, ldc, nb, g, 32 * g, N, K, 0, nullptr, nullptr, st, nullptr, nullptr, 0, M);
    } else
        launch_gemm_nt(A, lda, Bt, ldb, bias, C, ldc, M, N, K, st);
}

// detector activations carved from a workspace
struct DetBufs {
    float* xm;        // [NF][Mp]
    float* x0;        // [NP][Mp]
    std::vector<float*> act;    // [NP][C_l+1]
    std::vector<float*> rstd;   // [B][C_l+1]
    std::vector<float*> stash;  // [NP][C_l+1] pre-activations of a variant's block (det_needs_stash), else null
    float *mstats, *gstat, *mpart;   // mel statistics [B][Mp][4], [B][4], chunk partials [B][mstride][2 Mp]
    int mstride;
    float* pred;      // [B][nbits]
    float* zpart;     // split-K partial slabs of the last conv [zpart_slabs][NP][C_last]
    // per-clip partial maxima [B][64] for the f16 two-term GEMM's scales: of x0 (index 0) and of act[l] (index l + 1); of
    // dL/dZ_l in gmax[l & 1]
    std::vector<float*> amax;
    float* gmax[2];
    // a detector of temporal convolutions: the unfolded rows of the block at hand [NP][tk max_cin], forward (U) and backward
    // (dL/dU) alike -- the weights are frozen, so U is not kept; else null
    float* unf = nullptr;
};
constexpr int kTailSplit = 4;
// slabs of split-K partials of the last conv: 4 from the split-K GEMM, Cin/128 from the fused forward epilogue
static int zpart_slabs(const aware_detector* d) {
    const int s = d->n_layers >= 1 ? d->ch[d->n_layers - 1] / 128 : 0;
    return s > kTailSplit ? s : kTailSplit;
}
// Workspace carving.  Each entry point carves its workspace in one function, and its *_workspace_bytes runs the same
// function on a Carver without a base, which only counts.
static void carve_det(Carver& c, const aware_batch* b, const aware_detector* d, DetBufs& o) {
    const int Mp = d->ch[0];
    o.act.assign(d->n_layers, nullptr); o.rstd.assign(d->n_layers, nullptr); o.stash.assign(d->n_layers, nullptr);
    o.amax.assign(d->n_layers + 1, nullptr);
    o.xm = c.take<float>((size_t)b->NF * Mp);
    o.x0 = c.take<float>((size_t)b->NP * Mp);
    for (int l = 0; l < d->n_layers; ++l) {
        o.act[l] = c.take<float>((size_t)b->NP * d->ch[l + 1]);
        o.rstd[l] = c.take<float>((size_t)b->B * d->ch[l + 1]);
        o.stash[l] = det_needs_stash(d) ? c.take<float>((size_t)b->NP * d->ch[l + 1]) : nullptr;
    }
    o.mstats = c.take<float>((size_t)b->B * Mp * 4);
    o.gstat = c.take<float>((size_t)b->B * 4);
    o.mstride = (b->max_frames + 31) / 32;
    o.mpart = c.take<float>((size_t)b->B * o.mstride * 2 * Mp);
    o.pred = c.take<float>((size_t)b->B * d->nbits);
    o.zpart = c.take<float>((size_t)zpart_slabs(d) * b->NP * d->ch[d->n_layers]);
    for (int l = 0; l <= d->n_layers; ++l) o.amax[l] = c.take<float>((size_t)b->B * 64);
    o.gmax[0] = c.take<float>((size_t)b->B * 64);
    o.gmax[1] = c.take<float>((size_t)b->B * 64);
    o.unf = d->taps ? c.take<float>((size_t)b->NP * d->tk * d->max_cin) : nullptr;
}

// number of 32-row groups per clip when the fused clip-aligned GEMM applies (uniform batch,
// at most 128 pooled rows per clip), else 0
static int clip_tile_groups(const aware_batch* b) {
    if (!b->uniform_tp) return 0;
    const int g = (b->uniform_tp + 31) / 32;
    return (g >= 1 && g <= 4) ? g : 0;
}

// fewer clips than this: the per-clip mel front kernel would leave most CUs idle; the two-launch form wins
constexpr int kMelFrontMinClips = 192;
// fewer workgroups than this: the latency variant of the bf16x3 kernel serves the conv block (gemm_x3.hip, kSmallGrid)
constexpr int kH2MinGrid = 128;
// The wide form of the f16 two-term kernel (gemm_h2.hip, tile 2: 256-column slabs, 256 threads, two waves per SIMD) needs a
// grid of at least this many workgroups: the chip holds 512 of them at a time (256 CUs x 2), and below one full round the
// 128-column form's twice as many, half as heavy workgroups spread better.  Measured inside the embed loop on 3 s clips (ms per
// iteration, 128-column form / wide form everywhere / this rule): 256 clips (512 and 1024 workgroups) 0.987 / 0.954 / 0.955;
// 128 clips (256 and 512) 0.559 / 0.545 / 0.541 -- the 256-workgroup launches are better left narrow; 64 clips (128 and 256)
// 0.340 / 0.366 / 0.340.  The crossover lies between 256 and 512 workgroups.  DESIGN.md section 4.  (With the wide form's
// row-major epilogue: 0.976 / 0.922 / 0.921, 0.552 / 0.531 / 0.525, 0.339 / 0.366 / 0.338 -- the crossover has not moved.)
constexpr int kH2WideMinGrid = 512;
// conv_tile: aware_embed_config::conv_tile (0 automatic, 1 the 128-column form, 2 the wide form wherever it can run).
// Returns the `tile` of launch_gemm_clip_h2 for a [B clips of nwm row groups] x N x K launch.
static int h2_conv_tile(int conv_tile, int B, int nwm, int N, int K) {
    if (conv_tile == 1 || !gemm_clip_h2_wide_supported(nwm, N, K, K)) return 1;
    if (conv_tile == 2) return 2;
    return (N / kH2WideTile) * B >= kH2WideMinGrid ? 2 : 1;
}

// The kernels of one detector call, chosen once by det_plan and launched by det_forward / det_forward_backward.
enum class MelFwd : unsigned char {
    Folded,   // the analysis kernel left the raw mel tile in xm: the norms and pooling only
    Front,    // mel GEMM, norms and pooling in one launch (launch_mel_front_x3)
    Gemm,     // mel GEMM, then the norms and pooling (launch_mel_norm_fwd)
};
// a conv block's forward (GEMM + norm + activation), or its data-gradient GEMM with the previous block's norm and activation
// backward fused in where the kind is not Plain
enum class Conv : unsigned char {
    Plain,         // gemm_plain, then launch_norm_act (forward) / its backward for block l - 1 (next layer down)
    ClipF32,       // clip-aligned GEMM, norm / activation in the epilogue (uniform batch, f32 MFMA)
    ClipX3,        // the same on the bf16 three-term kernel
    ClipH2,        // the same on the f16 two-term kernel (per-clip operand scales from partial maxima)
    RaggedX3,      // ragged batch / long clips, clips walked in chunks of rows: bf16 three-term
    RaggedH2,      // the same on the f16 two-term kernel
    SplitK,        // forward of a skinny last block: split-K partial slabs, summed by the tail read-out
    ReadoutGrad,   // data gradient of the last block from the tail's pitch-64 dL/dZ (launch_readout_grad_ragged_x3)
    MelBack,       // data gradient of block 0 + the mel stage's backward in one launch (launch_mel_back_x3)
};
enum class Readout : unsigned char {
    X3,     // the last block, read-out, loss and their backward in one kernel (launch_readout_x3)
    Tail,   // sum of the split-K slabs + read-out (launch_tail)
    Wide,   // more than 64 channels: one workgroup per clip (launch_readout_wide)
    Head,   // launch_head
};
struct DetPlan {
    int pipe = 0, nwm = 0;    // conv pipe (aware_embed_config::conv_pipe); clip_tile_groups
    MelFwd mel = MelFwd::Gemm;
    bool mel_amax = false;    // the mel kernel is handed amax[0]
    bool mag_grad = true;     // the backward ends with the GEMM to dL/d|S| (else the caller expands dL/d(mel) itself)
    int n_fwd = 0;            // blocks the forward runs (the fused read-out computes the last one itself)
    int top = 0;              // first block the backward loop differentiates
    Readout readout = Readout::Head;
    bool tail_k64 = false;    // the tail writes dL/dZ of the last block with a row pitch of 64, for Conv::ReadoutGrad
    Conv fwd[kMaxLayers] = {}, bwd[kMaxLayers] = {};
    // Conv::ClipH2 launches: the form of the kernel (h2_conv_tile: 1 = 128-column slabs, 2 = wide), else 0
    unsigned char fwd_tile[kMaxLayers] = {}, bwd_tile[kMaxLayers] = {};
    // x_max[l]: the kernel that writes block l's input also leaves its per-clip maxima in amax[l], for an f16 two-term block
    // l (otherwise that block launches the maxima kernel first); g_max[l]: the same for dL/dZ_l in gmax[l & 1]
    bool x_max[kMaxLayers + 1] = {}, g_max[kMaxLayers] = {};
    // dz[l]: the backward reaches block l with dL/dZ_l (its norm and activation backward fused into the kernel before), else
    // with dL/dA_l and launches the backward of launch_norm_act first
    bool dz[kMaxLayers] = {};
};
static bool is_h2(Conv k) { return k == Conv::ClipH2 || k == Conv::RaggedH2; }

// readout: aware_embed_config::readout (1: never the fused read-out); training: the parameter gradients are wanted too;
// mel_folded: the analysis kernel writes the raw mel tile (xm); mel_grad_only: the backward stops at dL/d(mel)
static DetPlan det_plan(const aware_detector* d, const aware_batch* b, int pipe, int readout, bool training, bool mel_folded,
                        bool mel_grad_only, int conv_tile = 0) {
    DetPlan p;
    const int nl = d->n_layers;
    const std::vector<int>& ch = d->ch;
    const bool card = d->card_arch;        // the fused kinds serve the model card's blocks only
    const int nwm = clip_tile_groups(b);
    p.pipe = pipe; p.nwm = nwm;
    // uniform batch that fills the chip with one workgroup per clip: the whole mel block in one launch, and its backward with
    // block 0's data gradient
    bool same_T = true;
    for (int i = 1; i < b->B; ++i) same_T = same_T && b->T[i] == b->T[0];
    const bool mel_front = !d->pooled && pipe != 1 && d->n_mels == 128 && d->melTpk && same_T && b->B >= kMelFrontMinClips &&
                           mel_front_x3_supported(b->T[0], d->stride, d->stride);
    p.mel = mel_folded ? MelFwd::Folded : mel_front ? MelFwd::Front : MelFwd::Gemm;
    p.mel_amax = p.mel == MelFwd::Front || (p.mel == MelFwd::Folded && pipe == 0 && nwm);
    p.mag_grad = !mel_grad_only;
    // one kernel for the last conv block, the BRH head, the loss, their backward and the data gradient of the last conv
    // (uniform batches, bf16x3 configuration); otherwise split-K GEMM + tail kernel + data-gradient GEMM
    const bool fused_readout = card && readout == 0 && !training && pipe != 1 && nwm && nl >= 2 && d->lastpk &&
                               ch[nl] == 2 * d->nbits && readout_x3_supported(nwm, ch[nl - 1], ch[nl]) && d->wpk[nl - 2] &&
                               gemm_clip_x3_supported(nwm, ch[nl - 1], ch[nl - 2], ch[nl - 2]);
    p.n_fwd = fused_readout ? nl - 1 : nl;
    for (int l = 0; l < nl; ++l) {
        const int ci = ch[l], co = ch[l + 1];
        Conv k = Conv::Plain;
        if (!card) {
        } else if (l == nl - 1 && co <= 64 && b->max_frames / 2 <= 320) {
            k = Conv::SplitK;
        } else if (nwm && co >= 128) {
            if (pipe == 0 && d->wh2[l] && (co / 128) * b->B >= kH2MinGrid && gemm_clip_h2_supported(nwm, co, ci, ci))
                k = Conv::ClipH2;
            else if (pipe != 1 && d->wpk[l] && gemm_clip_x3_supported(nwm, co, ci, ci))
                k = Conv::ClipX3;
            else
                k = Conv::ClipF32;
        } else if (pipe == 0 && !nwm && d->wh2[l] && co >= 128 && gemm_clip_h2_supported(1, co, ci, ci)) {
            k = Conv::RaggedH2;
        } else if (pipe != 1 && !nwm && co >= 128 && d->wpk[l] && gemm_clip_x3_supported(1, co, ci, ci)) {
            k = Conv::RaggedX3;
        }
        p.fwd[l] = k;
        p.fwd_tile[l] = k == Conv::ClipH2 ? (unsigned char)h2_conv_tile(conv_tile, b->B, nwm, co, ci) : 0;
    }
    // the clip form of the mel norm kernel leaves the maxima of x0 when handed amax[0]; the chunked form does not
    const bool mel_writes_max = p.mel == MelFwd::Front || (p.mel_amax && b->max_frames <= kMelClipFrames);
    for (int l = 0; l < p.n_fwd; ++l) p.x_max[l] = is_h2(p.fwd[l]) && (l == 0 ? mel_writes_max : is_h2(p.fwd[l - 1]));

    p.readout = fused_readout ? Readout::X3 : p.fwd[nl - 1] == Conv::SplitK ? Readout::Tail
              : ch[nl] > 64 ? Readout::Wide : Readout::Head;
    // ragged batch on the bf16x3 pipe: dL/dZ of the last block with a pitch of 64 (zero K padding), so that its data gradient
    // runs on the ragged conv kernel with the previous block's InstanceNorm + LeakyReLU backward fused
    p.tail_k64 = p.readout == Readout::Tail && !nwm && pipe != 1 && !training && nl >= 2 && d->lastTpk && ch[nl] <= 64 &&
                 ch[nl - 1] % 128 == 0;
    p.top = fused_readout ? nl - 2 : nl - 1;
    // the wide read-out writes dL/dZ of the last block on the card (dL/dA on a variant)
    const bool readout_dz = p.readout != Readout::Head && (p.readout != Readout::Wide || card);
    for (int l = p.top; l >= 0; --l) {
        const int ci = ch[l], co = ch[l + 1];
        p.dz[l] = l == p.top ? readout_dz : p.bwd[l + 1] != Conv::Plain;
        Conv k = Conv::Plain;
        if (!card) {
        } else if (nwm && l > 0 && ci >= 128) {
            if (pipe == 0 && d->wTh2[l] && (ci / 128) * b->B >= kH2MinGrid && gemm_clip_h2_supported(nwm, ci, co, co))
                k = Conv::ClipH2;
            else if (pipe != 1 && d->wTpk[l] && gemm_clip_x3_supported(nwm, ci, co, co))
                k = Conv::ClipX3;
            else
                k = Conv::ClipF32;
        } else if (l == nl - 1 && p.tail_k64) {
            k = Conv::ReadoutGrad;
        } else if (pipe == 0 && !nwm && l > 0 && d->wTh2[l] && ci >= 128 && co >= 128 && gemm_clip_h2_supported(1, ci, co, co)) {
            k = Conv::RaggedH2;
        } else if (pipe != 1 && !nwm && l > 0 && ci >= 128 && d->wTpk[l] && gemm_clip_x3_supported(1, ci, co, co)) {
            k = Conv::RaggedX3;
        } else if (l == 0 && mel_front && p.dz[0] && !training && d->wTpk[0] && co % 64 == 0 && d->n_mels == 128) {
            k = Conv::MelBack;
        }
        p.bwd[l] = k;
        p.bwd_tile[l] = k == Conv::ClipH2 ? (unsigned char)h2_conv_tile(conv_tile, b->B, nwm, ci, co) : 0;
        // the fused and wide read-outs, the f16 two-term kernels and the ragged read-out gradient leave the maxima of the
        // gradient they write for an f16 two-term consumer
        const bool writes_max = l == p.top ? p.readout == Readout::X3 || p.readout == Readout::Wide
                                           : is_h2(p.bwd[l + 1]) || p.bwd[l + 1] == Conv::ReadoutGrad;
        p.g_max[l] = is_h2(k) && writes_max;
    }
    return p;
}

// norm and activation of block l, in place on x: the conv's output (forward) or dL/dA_l (backward).  The model card's blocks are
// the struct's defaults with no stash and the default rows.
static NormActLaunch det_norm_act(const aware_detector* d, const aware_batch* b, const DetBufs& o, int l, float* x) {
    NormActLaunch L;
    L.norm = d->norm; L.act = d->act;
    L.x = x; L.out = o.act[l]; L.stash = o.stash[l]; L.rstd = o.rstd[l];
    L.scale = d->nscale[l]; L.shift = d->nshift[l];
    L.frame_off = b->d_frame_off; L.pool_off = b->d_pool_off;
    L.C = d->ch[l + 1]; L.B = b->B; L.max_pooled = b->max_frames / 2;
    L.rows = det_rows(d, l + 1);
    return L;
}

// forward through the network; mag [NF][stride] -> act, pred (mag is not read when the plan's mel stage is folded)
static int det_forward(const aware_detector* d, const aware_batch* b, const DetPlan& p, const float* mag, DetBufs& o,
                       hipStream_t st) {
    const int nl = d->n_layers, Mp = d->ch[0];
    if (p.mel == MelFwd::Front) {
        launch_mel_front_x3(mag, d->stride, d->melTpk, b->d_frame_off, b->d_pool_off, o.xm, o.x0, o.mstats, o.gstat, b->B, b->T[0],
                            d->stride, st, o.amax[0]);
    } else {
        if (p.mel == MelFwd::Gemm) {
            gemm_plain(p.pipe, mag, d->stride, d->melT, d->stride, d->melTpk, nullptr, o.xm, Mp, b->NF, Mp, d->stride, st);
            LAUNCHCHK(); PROF(K_GEMM);
        }
        if (d->pooled)      // any other initial pool: mel_pool_kernels.hip (no maxima: the staged route never asks for them)
            launch_mel_pool_fwd(o.xm, b->d_frame_off, b->d_pool_off, o.x0, o.mstats, o.gstat, o.mpart, o.mstride, b->B,
                                b->max_frames, d->n_mels, Mp, d->psize, d->pstride, st);
        else
            launch_mel_norm_fwd(o.xm, b->d_frame_off, b->d_pool_off, o.x0, o.mstats, o.gstat, o.mpart, o.mstride, b->B,
                                b->max_frames, d->n_mels, Mp, st, p.mel_amax ? o.amax[0] : nullptr);
    }
    LAUNCHCHK(); PROF(K_MELNORM);
    const float* x = o.x0;
    for (int l = 0; l < p.n_fwd; ++l) {
        const int ci = d->ch[l], co = d->ch[l + 1];
        float* amax_out = p.x_max[l + 1] ? o.amax[l + 1] : nullptr;
        const bool emit = p.readout == Readout::X3 && l == nl - 2;   // + split-K partials of the last conv (fused read-out)
        switch (p.fwd[l]) {
        case Conv::SplitK:
            launch_gemm_nt_splitk(x, ci, d->w[l], ci, o.zpart, co, b->NP, co, ci, kTailSplit, st);
            LAUNCHCHK(); PROF(K_GEMM);
            break;
        case Conv::ClipH2:
            if (!p.x_max[l]) { launch_clip_amax(x, ci, ci, 32 * p.nwm, b->B, o.amax[l], st); LAUNCHCHK(); PROF(K_MISC); }
            launch_gemm_clip_h2(x, ci, d->wh2[l], o.amax[l], amax_out, d->bias[l], o.act[l], co, b->B, p.nwm, b->uniform_tp, co, ci,
                                1, o.rstd[l], nullptr, st, emit ? d->lastpk : nullptr, emit ? o.zpart : nullptr, d->ch[nl],
                                p.fwd_tile[l]);
            LAUNCHCHK(); PROF(K_GEMM_X3_FWD);
            break;
        case Conv::ClipX3:
            launch_gemm_clip_x3(x, ci, d->wpk[l], d->bias[l], o.act[l], co, b->B, p.nwm, b->uniform_tp, co, ci, 1, o.rstd[l],
                                nullptr, st, emit ? d->lastpk : nullptr, emit ? o.zpart : nullptr, d->ch[nl]);
            LAUNCHCHK(); PROF(K_GEMM_X3_FWD);
            break;
        case Conv::ClipF32:
            launch_gemm_clip(x, ci, d->w[l], ci, d->bias[l], o.act[l], co, b->B, p.nwm, b->uniform_tp, co, ci, 1, o.rstd[l],
                             nullptr, st);
            LAUNCHCHK(); PROF(K_GEMM_CLIP_FWD);
            break;
        case Conv::RaggedH2:
            if (!p.x_max[l]) {
                launch_ragged_amax(x, ci, ci, b->d_frame_off, b->d_pool_off, b->B, o.amax[l], st);
                LAUNCHCHK(); PROF(K_MISC);
            }
            launch_gemm_ragged_h2(x, ci, d->wh2[l], o.amax[l], amax_out, d->bias[l], o.act[l], co, b->B, b->d_frame_off,
                                  b->d_pool_off, b->d_order, co, ci, 1, o.rstd[l], nullptr, st);
            LAUNCHCHK(); PROF(K_GEMM_X3_FWD);
            break;
        case Conv::RaggedX3:
            launch_gemm_ragged_x3(x, ci, d->wpk[l], d->bias[l], o.act[l], co, b->B, b->d_frame_off, b->d_pool_off, b->d_order, co,
                                  ci, 1, o.rstd[l], nullptr, st);
            LAUNCHCHK(); PROF(K_GEMM_X3_FWD);
            break;
        default:
            // conv + bias, then the block's norm and activation (a variant's pre-activation kept in the stash)
            // temporal convolutions: the same GEMM on the unfolded rows (K = tk ci), the norm over the block's own rows
            if (d->taps) {
                launch_conv_unfold(x, o.unf, b->d_frame_off, b->d_pool_off, ci, b->B, b->max_frames / 2, l, d->tk, d->ts, d->tp, st,
                                   d->psize, d->pstride);
                LAUNCHCHK(); PROF(K_MISC);
                gemm_plain(p.pipe, o.unf, d->tk * ci, d->w[l], d->tk * ci, d->wpk[l], d->bias[l], o.act[l], co, b->NP, co,
                           d->tk * ci, st);
            } else
                gemm_plain(p.pipe, x, ci, d->w[l], ci, d->wpk[l], d->bias[l], o.act[l], co, b->NP, co, ci, st);
            LAUNCHCHK(); PROF(K_GEMM);
            launch_norm_act(det_norm_act(d, b, o, l, o.act[l]), false, st);
            LAUNCHCHK(); PROF(K_INLRELU);
        }
        x = o.act[l];
    }
    return AWARE_OK;
}

// read-out of a forward-only call: values [B][nbits]
static void readout_forward(const aware_detector* d, const aware_batch* b, const DetPlan& p, const DetBufs& o, float* values,
                            hipStream_t st) {
    const int nl = d->n_layers, C = d->ch[nl];
    if (p.readout == Readout::Tail)
        launch_tail(o.zpart, kTailSplit, (size_t)b->NP * C, d->bias[nl - 1], b->d_frame_off, b->d_pool_off, nullptr, values,
                    nullptr, nullptr, nullptr, nullptr, nullptr, 0, d->nbits, b->B, b->max_frames / 2, st, nullptr, 0, C);
    else if (p.readout == Readout::Wide)
        launch_readout_wide(o.act[nl - 1], C, b->d_frame_off, b->d_pool_off, nullptr, nullptr, values, nullptr, nullptr, nullptr,
                            nullptr, nullptr, nullptr, 0, d->nbits, b->B, st, nullptr, d->final_act, false, det_rows(d, nl));
    else
        launch_head(o.act[nl - 1], b->d_frame_off, b->d_pool_off, nullptr, values, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                    d->nbits, b->B, st, nullptr, d->final_act, C, det_rows(d, nl));
}

// the general route's band kernels (loop_any.hip) for a plan and its batch
static BandLaunch band_launch(const aware_plan* plan, const aware_batch* b) {
    BandLaunch L;
    L.NF = b->NF; L.B = b->B; L.frame_off = b->d_frame_off; L.sstride = plan->gdev.stride;
    L.band_lo = plan->dev.band_lo; L.nband = plan->dev.nband; L.bstride = plan->dev.stride;
    return L;
}
// a general plan, its batch and a detector created for it: one geometry, one band layout
static bool gen_loop_matches(const aware_plan* plan, const aware_batch* b, const aware_detector* d) {
    return plan->band_ok && gen_batch_matches(plan, b) && d->general && d->n_fft == plan->n_fft &&
           d->band_lo == plan->dev.band_lo && d->nband == plan->dev.nband && d->stride == plan->dev.stride;
}

// aware_detect: the detector's buffers, the band magnitudes and the analysis's partial maxima; a general batch also the
// spectrum the band magnitudes are taken from
static void carve_detect(Carver& c, const aware_batch* b, const aware_detector* d, DetBufs& o, float*& mag,
                         unsigned long long*& pmax, cf*& spec) {
    carve_det(c, b, d, o);
    mag = c.take<float>((size_t)b->NF * d->stride);
    pmax = c.take<unsigned long long>((size_t)b->B * b->pstride);
    spec = b->general ? c.take<cf>((size_t)b->NF * gen_stride(b->g_nfft)) : nullptr;
}
extern "C" size_t aware_detect_workspace_bytes(const aware_batch* b, const aware_detector* d) {
    if (!b || !d) return 0;
    Carver c(nullptr, 0);
    DetBufs o;
    float* mag;
    unsigned long long* pmax;
    cf* spec;
    carve_detect(c, b, d, o, mag, pmax, spec);
    return c.off;
}

extern "C" int aware_detector_forward(const aware_detector* d, const aware_batch* b, const float* mag, float* values,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    if (!d || !b || b->general || !mag || !values || !workspace) return AWARE_E_BADARG;
    if (!det_clips_ok(d, b)) return AWARE_E_BADARG;           // a clip too short for the detector's pool or temporal convolutions
    hipStream_t st = (hipStream_t)stream;
    Carver c(workspace, workspace_bytes);
    DetBufs o;
    carve_det(c, b, d, o);
    if (!c.ok) return AWARE_E_WORKSPACE;
    for (int l = 0; l < d->n_layers; ++l) o.stash[l] = nullptr;      // forward only: no backward reads the pre-activations
    const DetPlan p = det_plan(d, b, 0, 1, false, false, false);
    int rc = det_forward(d, b, p, mag, o, st);
    if (rc) return rc;
    readout_forward(d, b, p, o, values, st);
    LAUNCHCHK();
    return AWARE_OK;
}

extern "C" int aware_detect(const aware_plan* plan, const aware_detector* d, const aware_batch* b, const float* audio,
                            float* values, void* workspace, size_t workspace_bytes, void* stream) {
    if (!plan || !d || !b || !audio || !values || !workspace) return AWARE_E_BADARG;
    if (plan->general && !plan->loop) return AWARE_E_UNSUPPORTED;          // a plan for the transforms alone
    if (plan->general ? !gen_loop_matches(plan, b, d) : (b->general || d->general)) return AWARE_E_BADARG;
    // the magnitude rows are carved at the detector's stride and written at the plan's: one band layout
    if (d->band_lo != plan->dev.band_lo || d->nband != plan->dev.nband || d->stride != plan->dev.stride) return AWARE_E_BADARG;
    if (!det_clips_ok(d, b)) return AWARE_E_BADARG;           // a clip too short for the detector's pool or temporal convolutions
    hipStream_t st = (hipStream_t)stream;
    Carver c(workspace, workspace_bytes);
    DetBufs o;
    float* mag;
    unsigned long long* pmax;
    cf* spec;
    carve_detect(c, b, d, o, mag, pmax, spec);
    if (!c.ok) return AWARE_E_WORKSPACE;
    for (int l = 0; l < d->n_layers; ++l) o.stash[l] = nullptr;
    int rc;
    if (plan->general) {
        // the general route: normalised spectrum (stft_any.hip), then its band magnitudes in the detector's layout
        rc = gen_stft(plan, b, audio, 1, spec, pmax, st);
        if (rc == AWARE_OK) { launch_band_mag(band_launch(plan, b), spec, mag, nullptr, true, st); LAUNCHCHK(); }
    } else
        rc = aware_stft_band(plan, b, audio, 1, mag, nullptr, pmax, stream);
    if (rc) return rc;
    const DetPlan p = det_plan(d, b, 0, 1, false, false, false);
    rc = det_forward(d, b, p, mag, o, st);
    if (rc) return rc;
    readout_forward(d, b, p, o, values, st);
    LAUNCHCHK();
    return AWARE_OK;
}

// Detector forward (multibit_detector_net.py:109-140), loss / gradient seed at the read-out, and the backward pass
// down to dL/d(band magnitudes) (data gradients only: the weights are frozen, multibit_embedder.py:76-77).
struct DetGradCtx {
    const float* target = nullptr;    // [B][n_bits]: bipolar watermark, or dL/dpred when loss_kind == AWARE_LOSS_EXTERNAL
    int loss_kind = 0;
    float* loss = nullptr;            // [B]
    float* best_loss = nullptr;       // [B] or null (no bookkeeping)
    int* improved = nullptr;
    int* step = nullptr;              // device step counter to advance, or null
    float *d1 = nullptr, *d2 = nullptr;   // gradient ping-pong [NP][maxc]
    float* gmag = nullptr;            // out: [NF][stride] (not written when the plan has no mag_grad: dL/d(mel) is left in
                                      // DetBufs::xm)
    const float* loss_add = nullptr;  // [B] per-clip term added to the loss before the best-loss bookkeeping (L1 part), or null
    // EXTENSION (detector training): also the parameter gradients dL/dW_l [Cout][Cin], dL/db_l [Cout]; tr1 / tr2 are
    // scratch for the transposed operands, [maxc][NP] each (plan made with training = true: the three-kernel read-out, which
    // writes dL/dZ of the last block to memory)
    float* const* wgrad = nullptr;
    float* const* bgrad = nullptr;
    float *tr1 = nullptr, *tr2 = nullptr;
};
static int det_forward_backward(const aware_detector* d, const aware_batch* b, const DetPlan& p, const float* mag, DetBufs& db,
                                const DetGradCtx& G, hipStream_t st) {
    const int nl = d->n_layers;
    int rc = det_forward(d, b, p, mag, db, st);
    if (rc) return rc;
    float* dA = G.d1;
    float* dB = G.d2;
    // maxima of dL/dZ_l for an f16 two-term data-gradient GEMM (written by the kernel before it, or read here first)
    auto gmax = [&](int l, bool wanted) { return wanted ? db.gmax[l & 1] : nullptr; };
    switch (p.readout) {
    case Readout::X3:
        // (dB, the other half of the gradient ping-pong, is free until the next data-gradient GEMM writes it: it holds the
        //  read-out's fragment image, readout_x3_image_bytes = 36 KB per 3 s clip, far below NP * maxc floats)
        launch_readout_x3(db.act[nl - 2], d->ch[nl - 1], db.zpart, d->ch[nl - 1] / 128, d->bias[nl - 1], d->lastTpk,
                          db.rstd[nl - 2], G.target, db.pred, G.loss, G.best_loss, G.improved, G.step, dA, b->B, p.nwm,
                          b->uniform_tp, d->ch[nl], d->nbits, G.loss_kind, st, G.loss_add, dB, gmax(nl - 2, p.g_max[nl - 2]));
        break;
    case Readout::Tail:
        launch_tail(db.zpart, kTailSplit, (size_t)b->NP * d->ch[nl], d->bias[nl - 1], b->d_frame_off, b->d_pool_off,
                    G.target, db.pred, G.loss, G.best_loss, G.improved, dA, G.step, G.loss_kind, d->nbits, b->B,
                    b->max_frames / 2, st, G.loss_add, p.tail_k64 ? 64 : 0, d->ch[nl]);
        break;
    case Readout::Wide:
        launch_readout_wide(db.act[nl - 1], d->ch[nl], b->d_frame_off, b->d_pool_off, db.rstd[nl - 1], G.target, db.pred, G.loss,
                            G.best_loss, G.improved, dA, gmax(nl - 1, p.g_max[nl - 1]), G.step, G.loss_kind, d->nbits, b->B, st,
                            G.loss_add, d->final_act, p.dz[nl - 1], det_rows(d, nl));
        break;
    default:
        launch_head(db.act[nl - 1], b->d_frame_off, b->d_pool_off, G.target, db.pred, G.loss, G.best_loss,
                    G.improved, dA, G.step, G.loss_kind, d->nbits, b->B, st, G.loss_add, d->final_act, d->ch[nl], det_rows(d, nl));
    }
    LAUNCHCHK(); PROF(K_HEAD);
    for (int l = p.top; l >= 0; --l) {
        const int ci = d->ch[l], co = d->ch[l + 1];
        if (!p.dz[l]) {
            launch_norm_act(det_norm_act(d, b, db, l, dA), true, st);
            LAUNCHCHK(); PROF(K_INLRELU);
        }
        // dA = dL/dZ_l [NP][co] (zero in padding rows), X = input of the block [NP][ci]:  dW = dZ^T X as an NT GEMM over
        // the transposed operands (K = NP contiguous); db = column sums of dZ (zero up to rounding: the InstanceNorm
        // behind the convolution removes any per-channel constant)
        // (the last block's padding channels: only the caller's 2 * nbits rows of dW and db are written)
        // Each of the two is written where the caller asks for it, whether or not it asks for the other.
        const bool want_w = G.wgrad && G.wgrad[l], want_b = G.bgrad && G.bgrad[l];
        const int rows = l == nl - 1 ? 2 * d->nbits : co;
        if (want_w) {
            const float* X = l > 0 ? db.act[l - 1] : db.x0;
            launch_transpose(dA, G.tr1, b->NP, co, st);
            launch_transpose(X, G.tr2, b->NP, ci, st);
            launch_gemm_nt(G.tr1, b->NP, G.tr2, b->NP, nullptr, G.wgrad[l], ci, rows, ci, b->NP, st);
        }
        if (want_b) {
            if (rows == co) launch_colsum(dA, G.bgrad[l], b->NP, co, st);
            else {
                launch_colsum(dA, G.tr2, b->NP, co, st);      // tr2 is free once the GEMM above has read it
                HIPCHK(hipMemcpyAsync(G.bgrad[l], G.tr2, (size_t)rows * sizeof(float), hipMemcpyDeviceToDevice, st));
            }
        }
        if (want_w || want_b) { LAUNCHCHK(); PROF(K_MISC); }
        // the data gradient of block l; every kind but Plain also runs the backward of block l-1's norm and activation
        float* g_out = l > 0 ? gmax(l - 1, p.g_max[l - 1]) : nullptr;
        switch (p.bwd[l]) {
        case Conv::ClipH2:
            if (!p.g_max[l]) { launch_clip_amax(dA, co, co, 32 * p.nwm, b->B, db.gmax[l & 1], st); LAUNCHCHK(); PROF(K_MISC); }
            launch_gemm_clip_h2(dA, co, d->wTh2[l], db.gmax[l & 1], g_out, nullptr, dB, ci, b->B, p.nwm, b->uniform_tp, ci, co, 2,
                                db.rstd[l - 1], db.act[l - 1], st, nullptr, nullptr, 0, p.bwd_tile[l]);
            LAUNCHCHK(); PROF(K_GEMM_X3_BWD);
            break;
        case Conv::ClipX3:
            launch_gemm_clip_x3(dA, co, d->wTpk[l], nullptr, dB, ci, b->B, p.nwm, b->uniform_tp, ci, co, 2, db.rstd[l - 1],
                                db.act[l - 1], st);
            LAUNCHCHK(); PROF(K_GEMM_X3_BWD);
            break;
        case Conv::ClipF32:
            launch_gemm_clip(dA, co, d->wT[l], co, nullptr, dB, ci, b->B, p.nwm, b->uniform_tp, ci, co, 2, db.rstd[l - 1],
                             db.act[l - 1], st);
            LAUNCHCHK(); PROF(K_GEMM_CLIP_BWD);
            break;
        case Conv::ReadoutGrad:
            launch_readout_grad_ragged_x3(db.act[l - 1], ci, dA, d->lastTpk, db.rstd[l - 1], dB, b->d_frame_off, b->d_pool_off,
                                          b->d_order, b->B, st, g_out);
            LAUNCHCHK(); PROF(K_GEMM_X3_BWD);
            break;
        case Conv::RaggedH2:
            if (!p.g_max[l]) {
                launch_ragged_amax(dA, co, co, b->d_frame_off, b->d_pool_off, b->B, db.gmax[l & 1], st);
                LAUNCHCHK(); PROF(K_MISC);
            }
            launch_gemm_ragged_h2(dA, co, d->wTh2[l], db.gmax[l & 1], g_out, nullptr, dB, ci, b->B, b->d_frame_off, b->d_pool_off,
                                  b->d_order, ci, co, 2, db.rstd[l - 1], db.act[l - 1], st);
            LAUNCHCHK(); PROF(K_GEMM_X3_BWD);
            break;
        case Conv::RaggedX3:
            launch_gemm_ragged_x3(dA, co, d->wTpk[l], nullptr, dB, ci, b->B, b->d_frame_off, b->d_pool_off, b->d_order, ci, co, 2,
                                  db.rstd[l - 1], db.act[l - 1], st);
            LAUNCHCHK(); PROF(K_GEMM_X3_BWD);
            break;
        case Conv::MelBack:
            launch_mel_back_x3(dA, co, d->wTpk[0], b->d_frame_off, b->d_pool_off, db.xm, db.mstats, db.gstat, b->B, b->T[0], co, st);
            LAUNCHCHK(); PROF(K_MELNORM);
            break;
        default:
            // temporal convolutions: the GEMM to dL/dU [NP][tk ci], then the fold to dL/dX (the adjoint of the unfold)
            if (d->taps) {
                gemm_plain(p.pipe, dA, co, d->wT[l], co, d->wTpk[l], nullptr, db.unf, d->tk * ci, b->NP, d->tk * ci, co, st);
                LAUNCHCHK(); PROF(K_GEMM);
                launch_conv_fold(db.unf, dB, b->d_frame_off, b->d_pool_off, ci, b->B, b->max_frames / 2, l, d->tk, d->ts, d->tp, st,
                                 d->psize, d->pstride);
                LAUNCHCHK(); PROF(K_MISC);
            } else {
                gemm_plain(p.pipe, dA, co, d->wT[l], co, d->wTpk[l], nullptr, dB, ci, b->NP, ci, co, st);
                LAUNCHCHK(); PROF(K_GEMM);
            }
        }
        float* t = dA; dA = dB; dB = t;
    }
    const int Mp = d->ch[0];
    if (d->pooled) {
        launch_mel_pool_bwd(dA, db.xm, b->d_frame_off, b->d_pool_off, db.mstats, db.gstat, db.mpart, db.mstride, b->B,
                            b->max_frames, d->n_mels, Mp, d->psize, d->pstride, st);
        LAUNCHCHK(); PROF(K_MELNORM);
    } else if (p.bwd[0] != Conv::MelBack) {
        launch_mel_norm_bwd(dA, db.xm, b->d_frame_off, b->d_pool_off, db.mstats, db.gstat, db.mpart, db.mstride, b->B,
                            b->max_frames, d->n_mels, Mp, st);
        LAUNCHCHK(); PROF(K_MELNORM);
    }
    if (p.mag_grad) {
        gemm_plain(p.pipe, db.xm, Mp, d->melB, Mp, d->melBpk, nullptr, G.gmag, d->stride, b->NF, d->stride, Mp, st);
        LAUNCHCHK(); PROF(K_GEMM);
    }
    return AWARE_OK;
}

// aware_detector_backward, and with training the detector-training entry points: the gradient ping-pong, the transposed
// operands of the weight gradients, and the per-clip losses / dL/d|S| where the caller passes none (own_*)
static void carve_grad(Carver& c, const aware_batch* b, const aware_detector* d, DetBufs& o, DetGradCtx& G, bool training,
                       bool own_loss, bool own_gmag) {
    carve_det(c, b, d, o);
    G.d1 = c.take<float>((size_t)b->NP * d->maxc);
    G.d2 = c.take<float>((size_t)b->NP * d->maxc);
    if (training) {
        G.tr1 = c.take<float>((size_t)b->NP * d->maxc);
        G.tr2 = c.take<float>((size_t)b->NP * d->maxc);
    }
    if (own_loss) G.loss = c.take<float>(b->B);
    if (own_gmag) G.gmag = c.take<float>((size_t)b->NF * d->stride);
}
// training: the larger of the two entry points' own buffers, dL/d|S| of aware_detector_train_gradients with grad_mag NULL
// (aware_detector_weight_gradients carves the per-clip losses instead, B floats)
static size_t grad_bytes(const aware_batch* b, const aware_detector* d, bool training) {
    Carver c(nullptr, 0);
    DetBufs o;
    DetGradCtx G;
    carve_grad(c, b, d, o, G, training, !training, training);
    return c.off;
}

// detector forward + backward for the differentiable plug-in seam: values = net(mag), grad_mag = (d values / d mag)^T grad_values
extern "C" size_t aware_detector_backward_workspace_bytes(const aware_batch* b, const aware_detector* d) {
    if (!b || !d) return 0;
    return grad_bytes(b, d, false);
}
extern "C" int aware_detector_backward(const aware_detector* d, const aware_batch* b, const float* mag,
                                       const float* grad_values, float* values, float* grad_mag, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    if (!d || !b || b->general || !mag || !grad_values || !grad_mag || !workspace) return AWARE_E_BADARG;
    if (!det_clips_ok(d, b)) return AWARE_E_BADARG;           // a clip too short for the detector's pool or temporal convolutions
    hipStream_t st = (hipStream_t)stream;
    Carver c(workspace, workspace_bytes);
    DetBufs o;
    DetGradCtx G;
    carve_grad(c, b, d, o, G, false, true, false);
    if (!c.ok) return AWARE_E_WORKSPACE;
    G.target = grad_values; G.loss_kind = AWARE_LOSS_EXTERNAL; G.gmag = grad_mag;
    int rc = det_forward_backward(d, b, det_plan(d, b, 0, 0, false, false, false), mag, o, G, st);
    if (rc) return rc;
    if (values) HIPCHK(hipMemcpyAsync(values, o.pred, (size_t)b->B * d->nbits * sizeof(float), hipMemcpyDeviceToDevice, st));
    return AWARE_OK;
}

// EXTENSION (BASELINE north_star "gradients ... all-reduce"; the reference freezes the detector, multibit_embedder.py:76-77,
// and trains nothing): forward + backward of the network INCLUDING the parameter gradients, for a data-parallel detector
// training step -- the caller all-reduces grad_weights / grad_biases across ranks (RCCL) and applies its optimiser, then
// refreshes the device copy with aware_detector_update.  grad_weights / grad_biases: host arrays of n_layers device
// pointers ([Cout][Cin] and [Cout] f32; entries may be NULL).
extern "C" size_t aware_detector_train_workspace_bytes(const aware_batch* b, const aware_detector* d) {
    if (!b || !d) return 0;
    return grad_bytes(b, d, true);
}
static int detector_train_core(const aware_detector* d, const aware_batch* b, const float* mag, const float* target, int loss_kind,
                               float* loss_out, float* values, float* grad_mag, float* const* grad_weights,
                               float* const* grad_biases, void* workspace, size_t workspace_bytes, void* stream);

// The same with the loss evaluated inside (ONE forward + backward per step): target [B][n_bits] bipolar, loss_kind an
// AWARE_LOSS_* of the embed loop (no best-loss bookkeeping), loss_out dev [B] per-clip losses.  The gradients are those of the
// SUM of the per-clip losses (scale by 1 / clips in the optimiser step for their mean).  grad_mag may be NULL.
extern "C" int aware_detector_train_gradients(const aware_detector* d, const aware_batch* b, const float* mag, const float* target,
                                              int loss_kind, float* loss_out, float* values, float* grad_mag,
                                              float* const* grad_weights, float* const* grad_biases, void* workspace,
                                              size_t workspace_bytes, void* stream) {
    if (!d || !b || !mag || !target || !loss_out || !grad_weights || !workspace) return AWARE_E_BADARG;
    if (loss_kind < 0 || loss_kind > AWARE_LOSS_BER) return AWARE_E_BADARG;
    return detector_train_core(d, b, mag, target, loss_kind, loss_out, values, grad_mag, grad_weights, grad_biases, workspace,
                               workspace_bytes, stream);
}

extern "C" int aware_detector_weight_gradients(const aware_detector* d, const aware_batch* b, const float* mag,
                                               const float* grad_values, float* values, float* grad_mag,
                                               float* const* grad_weights, float* const* grad_biases, void* workspace,
                                               size_t workspace_bytes, void* stream) {
    if (!d || !b || !mag || !grad_values || !grad_mag || !grad_weights || !workspace) return AWARE_E_BADARG;
    return detector_train_core(d, b, mag, grad_values, AWARE_LOSS_EXTERNAL, nullptr, values, grad_mag, grad_weights, grad_biases,
                               workspace, workspace_bytes, stream);
}

static int detector_train_core(const aware_detector* d, const aware_batch* b, const float* mag, const float* target, int loss_kind,
                               float* loss_out, float* values, float* grad_mag, float* const* grad_weights,
                               float* const* grad_biases, void* workspace, size_t workspace_bytes, void* stream) {
    if (!d || !b || b->general) return AWARE_E_BADARG;
    if (!det_trainable(d)) return AWARE_E_UNSUPPORTED;   // the training extension serves the model card's network only
    if (d->stride != kFS) return AWARE_E_UNSUPPORTED;    // ... on a band of the narrow layout
    hipStream_t st = (hipStream_t)stream;
    Carver c(workspace, workspace_bytes);
    DetBufs o;
    DetGradCtx G;
    G.loss = loss_out; G.gmag = grad_mag;
    carve_grad(c, b, d, o, G, true, !loss_out, !grad_mag);
    if (!c.ok) return AWARE_E_WORKSPACE;
    // padding rows of the gradient ping-pong buffers take part in the row contraction: keep them finite
    HIPCHK(hipMemsetAsync(G.d1, 0, (size_t)b->NP * d->maxc * sizeof(float) * 2, st));
    G.target = target; G.loss_kind = loss_kind;
    G.wgrad = grad_weights; G.bgrad = grad_biases;
    // exact-f32 pipe and the three-kernel read-out for the training step
    int rc = det_forward_backward(d, b, det_plan(d, b, 1, 1, true, false, false), mag, o, G, st);
    if (rc) return rc;
    if (values) HIPCHK(hipMemcpyAsync(values, o.pred, (size_t)b->B * d->nbits * sizeof(float), hipMemcpyDeviceToDevice, st));
    return AWARE_OK;
}

// ---------------------------------------------------------------------------------------------
struct aware_embed {
    const aware_plan* plan;
    const aware_detector* det;
    const aware_batch* b;
    aware_embed_config cfg;
    DetBufs db;
    // spectral state [NF][256]
    float *coef, *lo, *hi, *mom, *vel, *best, *mag, *gmag;
    cf *P, *U;
    // signals [NS]
    float *yraw, *oob, *gy;
    float* gpad;          // [B][2][512] reflect-pad parts of the synthesis adjoint (streaming DSP kernels)
    // original coefficients (the streaming analysis adjoint recomputes the box from them; also the L1 term's reference);
    // loss push_extremes + L1 (EXTENSION): per-run partial sums of |c - c0|, per-clip loss term
    float* c0 = nullptr;
    double* pl1 = nullptr;
    float* l1term = nullptr;
    // gradient ping-pong [NP][maxc]
    float *d1, *d2;
    // scalars
    float *loss, *best_loss, *target;
    int *improved, *step;
    float4* sched;
    unsigned long long *pmaxA, *pmaxY;
    double* pdot;
    float hyp[4];
    hipGraph_t graph = nullptr, graphN = nullptr;
    hipGraphExec_t gexec = nullptr, gexecN = nullptr;
    hipStream_t cap = nullptr;        // private stream used only to record the graph
    int steps_done = 0;               // optimiser steps since aware_embed_begin (host mirror of *step)
    // optimiser / scheduler other than the model card's (aware_embed_set_optimizer): the step runs as its own launch
    struct {
        bool active = false;
        int kind = 0, plateau = 0, patience = 0;
        float hyp[8] = {0};
        double wd = 0, factor = 0, threshold = 0, min_lr = 0, eps = 0, lr0 = 0;
        double* d_tab = nullptr;      // [num_iterations][5]
        double* d_lr = nullptr;       // [B] per-clip learning rate (plateau)
        double* d_state = nullptr;    // [B][3] plateau state
        std::vector<double> lr_init, state_init;
    } opt;
    // attack-aware embedding (aware_embed_set_loop_attacks; EXTENSION): the chain and its buffers in the caller's second
    // workspace.  n == 0: the loop issues exactly the launches of the plain loop
    LoopChainState la;
    // attack mixtures (aware_embed_set_loop_mixture; EXTENSION): mix_n chains, one drawn per clip and step into mix_choice.
    // Every clip belongs to one chain at a step, so the chains share z, pmaxZ, psq, pdot, gpad0, seeds and u -- those of `la`,
    // whose n stays 0 -- and keep only what a backward pass needs from its forward pass (carve_chain_private)
    int mix_n = 0;
    LoopChainState mix[kMaxLoopChains];
    unsigned long long mix_thr[kMaxLoopChains] = {0};
    int* mix_choice = nullptr;                    // [B]
    int mix_rv = -1;                              // the chain with the reverberation (aware_embed_buffer 13), -1 without one
    // the general route (a general plan; gen_embed_iteration): full spectra [NF][spectrum stride] -- S0 the normalised
    // original, whose band columns every step overwrites with coef * U; S2 the analysis of the normalised synthesis, then
    // the gradient of the synthesis' input; GS the gradient of S2, zero outside the band -- and the two normalised
    // signals with the gradient of the first [NS]
    cf *S0 = nullptr, *S2 = nullptr, *GS = nullptr;
    float *y1 = nullptr, *y2 = nullptr, *gy1 = nullptr;
    // attack-aware embedding on the general route (aware_embed_set_general_chain; EXTENSION): the chain and its buffers in the
    // caller's second workspace.  n == 0: the loop issues exactly the launches of the plain general route
    GenChainState gc;
};

// the embed loop's workspace: the detector's buffers, then the loop state; iters: num_iterations, l1: the L1 term's buffers
static void carve_embed(Carver& c, const aware_batch* b, const aware_detector* det, int iters, bool l1, aware_embed* e) {
    carve_det(c, b, det, e->db);
    const size_t nsp = (size_t)b->NF * det->stride;
    if (b->general) {
        // the general route: band rows, three full spectra, five signals; no out-of-band residual, no reflect-pad parts and
        // no L1 term (they belong to the card kernels).  The step tables are carved at the longest loop aware_embed_create
        // accepts whatever `iters` is, so aware_embed_workspace_bytes is exact: one byte less is AWARE_E_WORKSPACE
        iters = 4096;
        const size_t nfull = (size_t)b->NF * gen_stride(b->g_nfft);
        e->coef = c.take<float>(nsp); e->lo = c.take<float>(nsp); e->hi = c.take<float>(nsp);
        e->mom = c.take<float>(nsp); e->vel = c.take<float>(nsp); e->best = c.take<float>(nsp);
        e->mag = c.take<float>(nsp); e->gmag = c.take<float>(nsp); e->c0 = c.take<float>(nsp);
        e->U = c.take<cf>(nsp); e->P = e->U;
        e->S0 = c.take<cf>(nfull); e->S2 = c.take<cf>(nfull); e->GS = c.take<cf>(nfull);
        e->yraw = c.take<float>(b->NS); e->y1 = c.take<float>(b->NS); e->y2 = c.take<float>(b->NS);
        e->gy = c.take<float>(b->NS); e->gy1 = c.take<float>(b->NS);
        e->oob = nullptr; e->gpad = nullptr;
        e->d1 = c.take<float>((size_t)b->NP * det->maxc); e->d2 = c.take<float>((size_t)b->NP * det->maxc);
        e->loss = c.take<float>(b->B); e->best_loss = c.take<float>(b->B);
        e->target = c.take<float>((size_t)b->B * det->nbits);
        e->improved = c.take<int>(b->B); e->step = c.take<int>(4);
        e->sched = c.take<float4>(iters + 1);
        e->pmaxA = c.take<unsigned long long>((size_t)b->B * b->pstride);
        e->pmaxY = c.take<unsigned long long>((size_t)b->B * b->pstride);
        e->pdot = nullptr;
        e->opt.d_tab = c.take<double>((size_t)iters * 5);
        e->opt.d_lr = c.take<double>(b->B);
        e->opt.d_state = c.take<double>((size_t)b->B * 3);
        return;
    }
    e->coef = c.take<float>(nsp); e->lo = c.take<float>(nsp); e->hi = c.take<float>(nsp);
    e->mom = c.take<float>(nsp); e->vel = c.take<float>(nsp); e->best = c.take<float>(nsp);
    e->mag = c.take<float>(nsp); e->gmag = c.take<float>(nsp);
    e->P = c.take<cf>(nsp); e->U = c.take<cf>(nsp);
    e->yraw = c.take<float>(b->NS); e->oob = c.take<float>(b->NS); e->gy = c.take<float>(b->NS);
    e->gpad = c.take<float>((size_t)b->B * 1024);
    e->d1 = c.take<float>((size_t)b->NP * det->maxc); e->d2 = c.take<float>((size_t)b->NP * det->maxc);
    e->loss = c.take<float>(b->B); e->best_loss = c.take<float>(b->B);
    e->target = c.take<float>((size_t)b->B * det->nbits);
    e->improved = c.take<int>(b->B); e->step = c.take<int>(4);
    e->sched = c.take<float4>(iters + 1);
    e->pmaxA = c.take<unsigned long long>((size_t)b->B * b->pstride);
    e->pmaxY = c.take<unsigned long long>((size_t)b->B * b->pstride);
    e->pdot = c.take<double>((size_t)b->B * b->pstride);
    e->c0 = c.take<float>(nsp);
    e->opt.d_tab = c.take<double>((size_t)iters * 5);
    e->opt.d_lr = c.take<double>(b->B);
    e->opt.d_state = c.take<double>((size_t)b->B * 3);
    if (l1) {
        e->pl1 = c.take<double>((size_t)b->B * b->pstride);
        e->l1term = c.take<float>(b->B);
    }
}
extern "C" size_t aware_embed_workspace_bytes(const aware_batch* b, const aware_detector* d) {
    if (!b || !d) return 0;
    Carver c(nullptr, 0);
    aware_embed e;
    carve_embed(c, b, d, 4096, true, &e);      // the largest loop aware_embed_create accepts, with the L1 term
    return c.off;
}

// torch.optim.NAdam's per-step scalars (torch/optim/nadam.py _single_tensor_nadam): mu_product lives in a float32
// tensor and is read back with .item()
static void nadam_coefficients(int s, double lr, double b1, double b2, double md, float& mu_product, float out[3]) {
    const double bc2 = 1.0 - pow(b2, (double)s);
    const double mu = b1 * (1.0 - 0.5 * pow(0.96, s * md));
    const double mu_next = b1 * (1.0 - 0.5 * pow(0.96, (s + 1) * md));
    mu_product = mu_product * (float)mu;
    const double mp = (double)mu_product;
    out[0] = (float)(-lr * (1.0 - mu) / (1.0 - mp));
    out[1] = (float)((-lr * mu_next) / (1.0 - mp * mu_next));
    out[2] = (float)bc2;
}
extern "C" int aware_nadam_coefficients(int step, float lr, float beta1, float beta2, float momentum_decay,
                                        float* mu_product_io, float* coef3) {
    if (step < 1 || !mu_product_io || !coef3) return AWARE_E_BADARG;
    nadam_coefficients(step, lr, beta1, beta2, momentum_decay, *mu_product_io, coef3);
    return AWARE_OK;
}
extern "C" int aware_nadam_clamp_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const float* lo,
                                      const float* hi, size_t n, const float* coef3, float beta1, float beta2, float eps,
                                      void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !coef3 || n < 1) return AWARE_E_BADARG;
    launch_nadam_clamp(param, grad, exp_avg, exp_avg_sq, lo, hi, n, coef3[0], coef3[1], coef3[2], beta1, beta2, eps,
                       (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}
extern "C" int aware_opt_clamp_step(int kind, float* param, const float* grad, float* state1, float* state2, const float* lo,
                                    const float* hi, size_t n, const float* coef4, const float* hyp8, void* stream) {
    if (kind < 0 || kind > 7 || !param || !grad || !state1 || !state2 || !coef4 || !hyp8 || n < 1) return AWARE_E_BADARG;
    launch_opt_clamp(kind, param, grad, state1, state2, lo, hi, n, coef4, hyp8, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}
extern "C" int aware_waveform_normalize_bwd(const float* in, const float* grad_out, float* grad_in, const int* off,
                                            const int* len, int B, void* stream) {
    if (!in || !grad_out || !grad_in || !off || !len || B < 1) return AWARE_E_BADARG;
    launch_normalize_bwd(in, grad_out, grad_in, off, len, B, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}
extern "C" int aware_polar_decompose(const void* spec, float* mag, float* phase, size_t n, void* stream) {
    if (!spec || !mag || n < 1) return AWARE_E_BADARG;
    launch_polar_decompose(spec, mag, phase, n, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}
extern "C" int aware_polar_decompose_bwd(const void* spec, const float* grad_mag, const float* grad_phase, void* grad_spec,
                                         size_t n, void* stream) {
    if (!spec || !grad_spec || (!grad_mag && !grad_phase) || n < 1) return AWARE_E_BADARG;
    launch_polar_decompose_bwd(spec, grad_mag, grad_phase, grad_spec, n, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}
extern "C" int aware_polar_assemble(const float* mag, const float* phase, void* spec, size_t n, void* stream) {
    if (!mag || !phase || !spec || n < 1) return AWARE_E_BADARG;
    launch_polar_assemble(mag, phase, spec, n, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}
extern "C" int aware_polar_assemble_bwd(const float* mag, const float* phase, const void* grad_spec, float* grad_mag,
                                        float* grad_phase, size_t n, void* stream) {
    if (!mag || !phase || !grad_spec || (!grad_mag && !grad_phase) || n < 1) return AWARE_E_BADARG;
    launch_polar_assemble_bwd(mag, phase, grad_spec, grad_mag, grad_phase, n, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

extern "C" int aware_embed_create(aware_embed** out, const aware_plan* plan, const aware_detector* det,
                                  const aware_batch* b, const aware_embed_config* cfg, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    if (!out || !plan || !det || !b || !cfg || !workspace) return AWARE_E_BADARG;
    if (plan->general && !plan->loop) return AWARE_E_UNSUPPORTED;          // a plan for the transforms alone
    if (plan->general ? !gen_loop_matches(plan, b, det) : (b->general || det->general)) return AWARE_E_BADARG;
    if (plan->general) {
        // torch.istft's NOLA condition for every clip, and at least one hop of output to analyse again
        if (!b->nola_ok) return AWARE_E_BADARG;
        for (int i = 0; i < b->B; ++i)
            if (b->out_len[i] < 1) return AWARE_E_BADARG;
    }
    if (cfg->num_iterations < 1 || cfg->num_iterations > 4096 || cfg->loss < 0 || cfg->loss > AWARE_LOSS_BCE ||
        cfg->loss == AWARE_LOSS_EXTERNAL)
        return AWARE_E_BADARG;
    // binary cross-entropy reads probabilities: torch raises on a prediction outside [0, 1], which only a sigmoid read-out rules out
    if (cfg->loss == AWARE_LOSS_BCE && det->final_act != kActSigmoid) return AWARE_E_UNSUPPORTED;
    if (cfg->conv_pipe < 0 || cfg->conv_pipe > 2 || cfg->readout < 0 || cfg->readout > 1 || cfg->mel < 0 || cfg->mel > 1)
        return AWARE_E_BADARG;
    if (cfg->dsp_path < 0 || cfg->dsp_path > 1 || cfg->conv_tile < 0 || cfg->conv_tile > 2) return AWARE_E_BADARG;
    // the detector's mel operands have the layout of the plan it was created for
    if (det->band_lo != plan->dev.band_lo || det->nband != plan->dev.nband || det->stride != plan->dev.stride) return AWARE_E_BADARG;
    if (!det_clips_ok(det, b)) return AWARE_E_BADARG;         // a clip too short for the detector's pool or temporal convolutions
    // the L1 term lives in the streaming DSP kernels only
    const bool l1 = cfg->loss == AWARE_LOSS_PUSH_L1;
    if (l1 && (plan->general || cfg->dsp_path != 0 || !stream_supported(plan->dev))) return AWARE_E_UNSUPPORTED;
    if (cfg->conv_tile == 2) {
        // the wide form was asked for: some conv launch of this session has to be able to take it
        const DetPlan p = det_plan(det, b, cfg->conv_pipe, cfg->readout, false, false, false, 2);
        bool any = false;
        for (int l = 0; l < det->n_layers; ++l) any = any || p.fwd_tile[l] == 2 || p.bwd_tile[l] == 2;
        if (!any) return AWARE_E_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    Building<aware_embed, aware_embed_destroy> e(new aware_embed());
    e->plan = plan; e->det = det; e->b = b; e->cfg = *cfg;
    Carver c(workspace, workspace_bytes);
    carve_embed(c, b, det, cfg->num_iterations, l1, e.get());
    if (!c.ok) return AWARE_E_WORKSPACE;
    const size_t nsp = (size_t)b->NF * plan->dev.stride;
    // columns nband..stride-1 of every spectral row are padding: zeroed once here, never written by the loop kernels
    HIPCHK(hipMemsetAsync(e->mag, 0, nsp * sizeof(float), st));
    HIPCHK(hipMemsetAsync(e->U, 0, nsp * sizeof(cf), st));
    if (e->gpad) HIPCHK(hipMemsetAsync(e->gpad, 0, (size_t)b->B * 1024 * sizeof(float), st));
    // general route: the gradient spectrum is zero outside the band, and only its band columns are ever written
    if (e->GS) HIPCHK(hipMemsetAsync(e->GS, 0, (size_t)b->NF * plan->gdev.stride * sizeof(cf), st));
    std::vector<float4> sc(cfg->num_iterations + 1);
    float mu_product = 1.0f;
    const double b1 = cfg->beta1, b2 = cfg->beta2;
    for (int s = 1; s <= cfg->num_iterations; ++s) {
        float c3[3];
        nadam_coefficients(s, cfg->lr, b1, b2, cfg->momentum_decay, mu_product, c3);
        sc[s - 1] = make_float4(c3[0], c3[1], c3[2], 0.f);
    }
    sc[cfg->num_iterations] = sc[cfg->num_iterations - 1];
    HIPCHK(hipMemcpyAsync(e->sched, sc.data(), sc.size() * sizeof(float4), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    e->hyp[0] = (float)(1.0 - b1); e->hyp[1] = (float)b2; e->hyp[2] = (float)(1.0 - b2); e->hyp[3] = cfg->eps;
    // measured tile choice for the ten GEMM shapes of this batch (a few ms, once per geometry;
    // every configuration gives bit-identical results)
    {
        HIPCHK(hipMemsetAsync(e->d1, 0, (size_t)b->NP * det->maxc * sizeof(float), st));
        HIPCHK(hipMemsetAsync(e->mag, 0, nsp * sizeof(float), st));
        // only the shapes the f32 kernel will actually serve (the bf16x3 kernel takes M % 32 == 0, N % 128 == 0, K % 64 == 0)
        auto f32_shape = [&](int M, int N, int K, int lda) {
            return !(cfg->conv_pipe != 1 && M % 32 == 0 && gemm_clip_x3_supported(1, N, K, lda));
        };
        const int S = det->stride;
        const int Mp = det->ch[0];
        if (f32_shape(b->NF, Mp, S, S)) gemm_autotune(e->mag, S, det->melT, S, e->db.xm, Mp, b->NF, Mp, S, st);
        if (f32_shape(b->NF, S, Mp, Mp)) gemm_autotune(e->db.xm, Mp, det->melB, Mp, e->gmag, S, b->NF, S, Mp, st);
        for (int l = 0; l < det->n_layers; ++l) {
            const int ci = det->ch[l], co = det->ch[l + 1];
            if (det->taps) {
                // temporal convolutions: the two GEMMs run on the unfolded rows, K and N = tk ci (the scratch is their operand)
                const int kc = det->tk * ci;
                if (l == 0) HIPCHK(hipMemsetAsync(e->db.unf, 0, (size_t)b->NP * det->tk * det->max_cin * sizeof(float), st));
                if (f32_shape(b->NP, co, kc, kc)) gemm_autotune(e->db.unf, kc, det->w[l], kc, e->d2, co, b->NP, co, kc, st);
                if (f32_shape(b->NP, kc, co, co)) gemm_autotune(e->d1, co, det->wT[l], co, e->db.unf, kc, b->NP, kc, co, st);
                continue;
            }
            if (f32_shape(b->NP, co, ci, ci)) gemm_autotune(e->d1, ci, det->w[l], ci, e->d2, co, b->NP, co, ci, st);
            if (f32_shape(b->NP, ci, co, co)) gemm_autotune(e->d1, co, det->wT[l], co, e->d2, ci, b->NP, ci, co, st);
        }
        HIPCHK(hipStreamSynchronize(st));
    }
    *out = e.release();
    return AWARE_OK;
}
// The third seam of the reference: optimiser / scheduler registries selected by YAML strings (embedding/optimizers.py:3-20,
// schedulers.py:3-16).  The host computes the per-step scalars of the chosen torch optimiser under the chosen learning-rate
// schedule (aware_amd/embedding/optimizers.py); the device applies them (opt_clamp_update, dsp_args.hpp).
extern "C" int aware_embed_set_optimizer(aware_embed* e, const aware_optimizer_config* oc, void* stream) {
    if (!e || !oc || oc->kind < 0 || oc->kind > 7 || !oc->table) return AWARE_E_BADARG;
    if (e->gexec) return AWARE_E_BADARG;                 // before the first aware_embed_iterate (the graphs are recorded then)
    if (oc->plateau && (!(oc->factor < 1.0) || oc->patience < 0)) return AWARE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int n = e->cfg.num_iterations, B = e->b->B;
    auto& o = e->opt;
    HIPCHK(hipMemcpyAsync(o.d_tab, oc->table, (size_t)n * 5 * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    o.kind = oc->kind; o.plateau = oc->plateau; o.patience = oc->patience;
    for (int i = 0; i < 8; ++i) o.hyp[i] = oc->hyp[i];
    o.wd = oc->weight_decay; o.factor = oc->factor; o.threshold = oc->threshold; o.min_lr = oc->min_lr; o.eps = oc->eps;
    o.lr0 = oc->lr0;
    o.lr_init.assign(B, oc->lr0);
    o.state_init.assign((size_t)B * 3, 0.0);
    for (int b = 0; b < B; ++b) o.state_init[3 * b] = (double)INFINITY;
    o.active = true;
    return AWARE_OK;
}

// Attack-aware embedding (EXTENSION): the chains' parser and the carving of their workspace are loop_chain.hpp's
static LoopDims loop_dims(const aware_batch* b) {
    LoopDims d;
    d.B = b->B; d.NS = b->NS; d.NF = b->NF; d.pstride = b->pstride; d.out_len = b->out_len.data();
    return d;
}
// W_2048^j, j < 1024, then W_4096^k, k <= 2048 (padded to 2056), from float64
static const std::vector<cf>& reverb_tables() {
    static const std::vector<cf> t = [] {
        std::vector<cf> v(kReverbTwHalf + kReverbBins, mk(0.f, 0.f));
        const double pi = 3.14159265358979323846;
        for (int j = 0; j < kReverbTwHalf; ++j) v[j] = mk((float)cos(-2.0 * pi * j / 2048.0), (float)sin(-2.0 * pi * j / 2048.0));
        for (int k = 0; k <= kReverbBlock; ++k)
            v[kReverbTwHalf + k] = mk((float)cos(-2.0 * pi * k / 4096.0), (float)sin(-2.0 * pi * k / 4096.0));
        return v;
    }();
    return t;
}
extern "C" size_t aware_embed_loop_attack_workspace_bytes(const aware_batch* b, int n_attacks) {
    if (!b || b->general || n_attacks < 1 || n_attacks > kMaxLoopAttacks) return 0;
    Carver c(nullptr, 0);
    LoopChainState la;
    carve_chain_shared(c, loop_dims(b), la);
    return c.off;
}
extern "C" size_t aware_embed_loop_attack_workspace_bytes_ex(const aware_batch* b, const aware_loop_attack_ex* attacks,
                                                             int n_attacks) {
    return (b && !b->general) ? loop_chain_workspace_bytes(loop_dims(b), attacks, n_attacks) : 0;
}
static void clear_loop_chain(aware_embed* e) {
    e->la.n = 0; e->la.z = nullptr; e->la.split = -1; e->la.pair_speed = -1; e->la.h = nullptr;
    e->mix_n = 0; e->mix_choice = nullptr; e->mix_rv = -1;
}
// what both setters do to a chain's buffers before the first step: the window of the overlap-add kinds (`hann`: the one a
// mixture's earlier chain fetched), and the reverberation's twiddles and zeroed responses (those of a clip that never draws
// the chain read as zeros)
static int init_chain_buffers(LoopChainState& la, const aware_batch* b, const float*& hann, hipStream_t st) {
    if (chain_has(la, AWARE_LOOP_TIME_STRETCH) || chain_has(la, AWARE_LOOP_PITCH_SHIFT)) {
        if (!hann && !(hann = stretch_window())) return AWARE_E_HIP;
    }
    la.hann = hann;
    if (chain_has(la, AWARE_LOOP_REVERBERATION)) {
        const std::vector<cf>& t = reverb_tables();
        HIPCHK(hipMemcpyAsync(la.tables, t.data(), t.size() * sizeof(cf), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(la.h, 0, (size_t)b->B * kReverbMaxIr * sizeof(float), st));
        HIPCHK(hipMemsetAsync(la.nh, 0, (size_t)b->B * sizeof(int), st));
    }
    if (chain_has(la, AWARE_LOOP_TIME_WARP)) {           // read only where the forward pass of the same step wrote them
        HIPCHK(hipMemsetAsync(la.warpR, 0, (size_t)b->B * la.kmax * sizeof(int), st));
        HIPCHK(hipMemsetAsync(la.warpA, 0, (size_t)b->B * la.kmax * sizeof(long long), st));
    }
    return AWARE_OK;
}
static int set_loop_attacks(aware_embed* e, const aware_loop_attack_ex* attacks, int n_attacks, bool ex,
                            const uint32_t* seeds, void* workspace, size_t workspace_bytes, void* stream) {
    if (!e || n_attacks < 0 || n_attacks > kMaxLoopAttacks) return AWARE_E_BADARG;
    if (e->gexec || e->la.locked) return AWARE_E_BADARG;          // before the first aware_embed_iterate, as aware_embed_set_optimizer
    if (n_attacks == 0) { clear_loop_chain(e); return AWARE_OK; }
    const aware_batch* b = e->b;
    if (b->general) return AWARE_E_UNSUPPORTED;                   // the stage kernels run on the card geometry only
    if (!attacks || !seeds || !workspace || ((uintptr_t)workspace & 255)) return AWARE_E_BADARG;
    auto la = e->la;
    la.gate = LoopGate();
    if (int rc = parse_loop_chain(loop_dims(b), attacks, n_attacks, ex, la)) return rc;
    Carver c(workspace, workspace_bytes);
    carve_loop_chain(c, loop_dims(b), la);
    if (!c.ok) return AWARE_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const float* hann = nullptr;
    if (int rc = init_chain_buffers(la, b, hann, st)) return rc;
    HIPCHK(hipMemsetAsync(la.gpad0, 0, (size_t)b->B * 1024 * sizeof(float), st));
    HIPCHK(hipMemcpyAsync(la.seeds, seeds, (size_t)b->B * sizeof(unsigned), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    la.n = n_attacks;
    e->la = la;
    e->mix_n = 0; e->mix_choice = nullptr; e->mix_rv = -1;          // a plain chain replaces a mixture
    return AWARE_OK;
}
extern "C" int aware_embed_set_loop_attacks(aware_embed* e, const aware_loop_attack* attacks, int n_attacks,
                                            const uint32_t* seeds, void* workspace, size_t workspace_bytes, void* stream) {
    aware_loop_attack_ex ex[kMaxLoopAttacks] = {};
    for (int j = 0; attacks && j < n_attacks && j < kMaxLoopAttacks; ++j) {
        ex[j].kind = attacks[j].kind; ex[j].prob = attacks[j].prob; ex[j].param[0] = attacks[j].param;
    }
    return set_loop_attacks(e, attacks ? ex : nullptr, n_attacks, false, seeds, workspace, workspace_bytes, stream);
}
extern "C" int aware_embed_set_loop_attacks_ex(aware_embed* e, const aware_loop_attack_ex* attacks, int n_attacks,
                                               const uint32_t* seeds, void* workspace, size_t workspace_bytes, void* stream) {
    return set_loop_attacks(e, attacks, n_attacks, true, seeds, workspace, workspace_bytes, stream);
}

// ---- the general route's chain (EXTENSION): the element-wise kinds at any geometry (loop_any_chain.hip);
// parser and carver are loop_any_chain.hpp's
extern "C" size_t aware_embed_general_chain_workspace_bytes(const aware_batch* b, const aware_loop_attack_ex* attacks, int n_attacks) {
    return (b && b->general) ? gen_chain_workspace_bytes(loop_dims(b), attacks, n_attacks) : 0;
}
extern "C" int aware_embed_set_general_chain(aware_embed* e, const aware_loop_attack_ex* attacks, int n_attacks, const uint32_t* seeds,
                                             void* workspace, size_t workspace_bytes, void* stream) {
    if (!e || n_attacks < 0 || n_attacks > kMaxLoopAttacks) return AWARE_E_BADARG;
    if (e->gexec || e->la.locked) return AWARE_E_BADARG;          // before the first aware_embed_iterate, as the card's setters
    const aware_batch* b = e->b;
    if (!b->general) return AWARE_E_UNSUPPORTED;                  // the card route has its own setters
    if (n_attacks == 0) { e->gc = GenChainState(); return AWARE_OK; }
    if (!attacks || !seeds || !workspace || ((uintptr_t)workspace & 255)) return AWARE_E_BADARG;
    GenChainState gc;
    if (int rc = parse_gen_chain(loop_dims(b), attacks, n_attacks, gc)) return rc;
    Carver c(workspace, workspace_bytes);
    carve_gen_chain(c, loop_dims(b), gc);
    if (!c.ok) return AWARE_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(gc.seeds, seeds, (size_t)b->B * sizeof(unsigned), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    e->gc = gc;
    return AWARE_OK;
}

// ---- attack mixtures (EXTENSION): one of several chains drawn per clip and step (loop_mix_kernels.hip)
extern "C" size_t aware_embed_loop_mixture_workspace_bytes(const aware_batch* b, const aware_loop_chain* chains, int n_chains) {
    return (b && !b->general) ? loop_mixture_workspace_bytes(loop_dims(b), chains, n_chains) : 0;
}
extern "C" int aware_embed_set_loop_mixture(aware_embed* e, const aware_loop_chain* chains, int n_chains, const uint32_t* seeds,
                                            void* workspace, size_t workspace_bytes, void* stream) {
    if (!e || n_chains < 0 || n_chains > kMaxLoopChains) return AWARE_E_BADARG;
    if (e->gexec || e->la.locked) return AWARE_E_BADARG;          // before the first aware_embed_iterate, as the chain's setter
    if (n_chains == 0) { clear_loop_chain(e); return AWARE_OK; }
    const aware_batch* b = e->b;
    if (b->general) return AWARE_E_UNSUPPORTED;                   // as the chain's setter
    if (!chains || !seeds || !workspace || ((uintptr_t)workspace & 255)) return AWARE_E_BADARG;
    LoopChainState shared, mix[kMaxLoopChains];
    unsigned long long thr[kMaxLoopChains];
    int rv = -1, *choice = nullptr;
    if (int rc = parse_loop_mixture(loop_dims(b), chains, n_chains, mix, thr, rv)) return rc;
    Carver c(workspace, workspace_bytes);
    carve_loop_mixture(c, loop_dims(b), shared, mix, n_chains, choice);
    if (!c.ok) return AWARE_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const float* hann = nullptr;
    for (int i = 0; i < n_chains; ++i) {
        mix[i].gate.choice = choice; mix[i].gate.chain = i;
        if (int rc = init_chain_buffers(mix[i], b, hann, st)) return rc;
    }
    HIPCHK(hipMemsetAsync(shared.gpad0, 0, (size_t)b->B * 1024 * sizeof(float), st));
    HIPCHK(hipMemcpyAsync(shared.seeds, seeds, (size_t)b->B * sizeof(unsigned), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)choice, -1, b->B, st));
    // a clip reaches a chain's stage only at the steps it draws the chain.  Every stage kernel is gated per clip, so the
    // signals in between are never read where they were not written; they start as zeros all the same
    HIPCHK(hipMemsetAsync(shared.z, 0, (size_t)b->NS * sizeof(float), st));
    if (shared.u) HIPCHK(hipMemsetAsync(shared.u, 0, (size_t)b->NS * sizeof(float), st));
    HIPCHK(hipStreamSynchronize(st));
    clear_loop_chain(e);                                           // a mixture replaces a plain chain
    const bool locked = e->la.locked;
    e->la = shared; e->la.n = 0; e->la.locked = locked;
    for (int i = 0; i < n_chains; ++i) { e->mix[i] = mix[i]; e->mix_thr[i] = thr[i]; }
    e->mix_n = n_chains; e->mix_choice = choice; e->mix_rv = rv;
    return AWARE_OK;
}
// the draw alone: choice[b] for B clips at `step`, weights on the host
extern "C" int aware_loop_mixture_draw(const uint32_t* seeds, int B, int step, const float* weights, int n_chains, int* choice,
                                       void* stream) {
    if (!seeds || !weights || !choice || B < 1 || n_chains < 1 || n_chains > kMaxLoopChains) return AWARE_E_BADARG;
    double sum = 0.0;
    for (int i = 0; i < n_chains; ++i) {
        if (!std::isfinite(weights[i]) || weights[i] < 0.f) return AWARE_E_BADARG;
        sum += (double)weights[i];
    }
    if (sum > 1.0 + 1e-6) return AWARE_E_BADARG;
    LoopMixDrawLaunch D;
    D.seeds = seeds; D.step_imm = step; D.B = B; D.n = n_chains; D.choice = choice;
    loop_mix_thresholds(weights, n_chains, D.thr);
    launch_loop_mix_draw(D, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

// ---- the convolution and the impulse-response draw alone (EXTENSION; attacks.Reverberation, tests) ------------------------
static void carve_convolve(Carver& c, int B, int kmax, int parts, ConvolveLaunch& L) {
    L.tables = c.take<cf>(kReverbTwHalf + kReverbBins);
    L.hspec = c.take<cf>((size_t)B * parts * kReverbBins);
    L.xspec = c.take<cf>((size_t)B * kmax * kReverbBins);
}
static int convolve_parts(int nh_max) { return std::min(kReverbParts, reverb_blocks(nh_max)); }
extern "C" size_t aware_convolve_workspace_bytes(int B, int max_len, long long total_len, int nh_max) {
    if (B < 1 || B > 65535 || max_len < 1 || nh_max < 1 || nh_max > kReverbMaxIr || total_len < max_len ||
        total_len > (long long)B * max_len)
        return 0;
    Carver c(nullptr, 0);
    ConvolveLaunch L;
    carve_convolve(c, B, reverb_blocks(max_len), convolve_parts(nh_max), L);
    return c.off;
}
extern "C" int aware_convolve(const float* in, const int* off, const int* len, int B, int max_len, const float* h,
                              int h_stride, const int* nh, int adjoint, float* out, void* workspace, size_t workspace_bytes,
                              void* stream) {
    if (!in || !off || !len || !h || !nh || !out || !workspace || ((uintptr_t)workspace & 255)) return AWARE_E_BADARG;
    if (B < 1 || B > 65535 || max_len < 1 || h_stride < 1 || h_stride > kReverbMaxIr || adjoint < 0 || adjoint > 1)
        return AWARE_E_BADARG;
    ConvolveLaunch L;
    L.B = B; L.kmax = reverb_blocks(max_len); L.parts = convolve_parts(h_stride);
    Carver c(workspace, workspace_bytes);
    carve_convolve(c, B, L.kmax, L.parts, L);
    if (!c.ok) return AWARE_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const std::vector<cf>& t = reverb_tables();
    HIPCHK(hipMemcpyAsync(const_cast<cf*>(L.tables), t.data(), t.size() * sizeof(cf), hipMemcpyHostToDevice, st));
    L.in = in; L.out = out; L.off = off; L.len = len; L.h = h; L.h_stride = h_stride; L.nh = nh; L.adjoint = adjoint;
    launch_convolve(L, st);
    LAUNCHCHK();
    return AWARE_OK;
}
extern "C" int aware_reverb_ir(const uint32_t* seeds, int B, int step, int entry, int n_lo, int n_hi, float drr_db, float* h,
                               int h_stride, int* nh, void* stream) {
    if (!seeds || !h || !nh || B < 1 || B > 65535 || step < 0 || entry < 0 || entry >= kMaxLoopAttacks) return AWARE_E_BADARG;
    if (n_lo < 2 || n_hi > kReverbMaxIr || n_lo > n_hi || h_stride < n_hi || !std::isfinite(drr_db)) return AWARE_E_BADARG;
    ReverbIrLaunch L;
    L.seeds = seeds; L.step_imm = step; L.entry = entry; L.B = B; L.n_lo = n_lo; L.n_hi = n_hi;
    L.gain = pow(10.0, (double)drr_db / 20.0); L.prob = 1.f; L.h = h; L.h_stride = h_stride; L.nh = nh;
    launch_reverb_ir(L, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

// the ragged signal array of a stand-alone attack entry point: 1 to 65535 clips, the longest of 1 to 2^30 samples
static bool ragged_args_ok(int B, int max_len) { return B >= 1 && B <= 65535 && max_len >= 1 && max_len <= (1 << 30); }

// ---- the in -> out resamplers alone: one argument list, one set of checks; `windowed`: the launch reads stretch_window() ------
static int resample_alone(void (*launch)(const ResampleLaunch&, hipStream_t), bool windowed, const float* in, const int* in_off,
                          const int* in_len, float* out, const int* out_off, const int* out_len, int B, int max_len, const int* m,
                          int adjoint, void* stream) {
    if (!in || !in_off || !in_len || !out || !out_off || !out_len || !m || in == out) return AWARE_E_BADARG;
    if (!ragged_args_ok(B, max_len) || adjoint < 0 || adjoint > 1) return AWARE_E_BADARG;
    ResampleLaunch L;
    if (windowed && !(L.window = stretch_window())) return AWARE_E_HIP;
    L.in = in; L.out = out; L.B = B; L.adjoint = adjoint; L.max_len = max_len; L.m = m;
    L.x_off = in_off; L.x_len = in_len; L.z_off = out_off; L.z_len = out_len;
    launch(L, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}
// the speed change (EXTENSION; attacks.SpeedChange, tests)
extern "C" int aware_speed_change(const float* in, const int* in_off, const int* in_len, float* out, const int* out_off,
                                  const int* out_len, int B, int max_len, const int* m, int adjoint, void* stream) {
    return resample_alone(launch_speed_change, false, in, in_off, in_len, out, out_off, out_len, B, max_len, m, adjoint, stream);
}
// the time stretch (EXTENSION; attacks.OverlapAddStretch, tests)
extern "C" int aware_stretch_ola(const float* in, const int* in_off, const int* in_len, float* out, const int* out_off,
                                 const int* out_len, int B, int max_len, const int* m, int adjoint, void* stream) {
    return resample_alone(launch_time_stretch, true, in, in_off, in_len, out, out_off, out_len, B, max_len, m, adjoint, stream);
}
// the pitch shift (EXTENSION; attacks.OverlapAddPitchShift, tests)
extern "C" int aware_pitch_shift_ola(const float* in, const int* in_off, const int* in_len, float* out, const int* out_off,
                                     const int* out_len, int B, int max_len, const int* m, int adjoint, void* stream) {
    return resample_alone(launch_pitch_shift, true, in, in_off, in_len, out, out_off, out_len, B, max_len, m, adjoint, stream);
}

// ---- the sample deletion alone (EXTENSION; runtime.delete_samples, tests) --------------------------------------------------
extern "C" int aware_delete_samples(const float* in, const int* off, const int* len, int B, int max_len, const int* start,
                                    const int* k, float* out, int adjoint, void* stream) {
    if (!in || !off || !len || !start || !k || !out || in == out) return AWARE_E_BADARG;
    if (!ragged_args_ok(B, max_len) || adjoint < 0 || adjoint > 1) return AWARE_E_BADARG;
    DeleteLaunch L;
    L.in = in; L.out = out; L.B = B; L.adjoint = adjoint; L.off = off; L.len = len; L.max_len = max_len; L.start = start; L.k = k;
    launch_delete_samples(L, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

// ---- the tiled excerpt alone (EXTENSION; attacks.ExcerptTile, runtime.excerpt_tile, tests) ----------------------------------
extern "C" int aware_excerpt_tile(const float* in, const int* off, const int* len, int B, int max_len, const int* start,
                                  const int* length, float* out, int adjoint, void* stream) {
    if (!in || !off || !len || !start || !length || !out || in == out) return AWARE_E_BADARG;
    if (!ragged_args_ok(B, max_len) || adjoint < 0 || adjoint > 1) return AWARE_E_BADARG;
    ExcerptLaunch L;
    L.in = in; L.out = out; L.B = B; L.adjoint = adjoint; L.off = off; L.len = len; L.max_len = max_len; L.start = start; L.length = length;
    launch_excerpt_tile(L, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

// ---- the time warp alone (EXTENSION; attacks.TimeWarp, attacks.Flutter, runtime.time_warp, tests) --------------------------
extern "C" int aware_time_warp(const float* in, const int* off, const int* len, int B, int max_len, const int* e, const int* ph,
                               const int* rates, int stride, int* table_r, long long* table_a, float* out, int adjoint, void* stream) {
    if (!in || !off || !len || !e || !ph || !rates || !table_r || !table_a || !out || in == out) return AWARE_E_BADARG;
    if (!ragged_args_ok(B, max_len) || stride < 3 || adjoint < 0 || adjoint > 1) return AWARE_E_BADARG;
    WarpLaunch L;
    L.in = in; L.out = out; L.B = B; L.adjoint = adjoint; L.table_r = table_r; L.table_a = table_a; L.stride = stride;
    L.off = off; L.len = len; L.max_len = max_len; L.e = e; L.ph = ph; L.rates = rates;
    launch_time_warp(L, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

// ---- the band filter alone (EXTENSION; attacks.BandFilter, runtime.band_filter, tests) -------------------------------------
extern "C" int aware_band_filter(const float* in, const int* off, const int* len, int B, int max_len, const int* response,
                                 const int* c1, const int* c2, float* out, float* taps, void* stream) {
    if (!in || !off || !len || !response || !c1 || !c2 || !out || in == out) return AWARE_E_BADARG;
    if (!ragged_args_ok(B, max_len)) return AWARE_E_BADARG;
    FilterLaunch L;
    L.in = in; L.out = out; L.B = B; L.off = off; L.len = len; L.max_len = max_len; L.response = response; L.c1 = c1; L.c2 = c2;
    L.taps = taps;
    launch_band_filter(L, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

// ---- the frequency shift alone (EXTENSION; attacks.FrequencyShift, runtime.frequency_shift, tests) --------------------------
extern "C" int aware_frequency_shift(const float* in, const int* off, const int* len, int B, int max_len, const int* d,
                                     const int* p0, int adjoint, float* out, void* stream) {
    if (!in || !off || !len || !d || !p0 || !out || in == out) return AWARE_E_BADARG;
    if (!ragged_args_ok(B, max_len) || adjoint < 0 || adjoint > 1) return AWARE_E_BADARG;
    ShiftLaunch L;
    L.in = in; L.out = out; L.B = B; L.adjoint = adjoint; L.off = off; L.len = len; L.max_len = max_len; L.d = d; L.p0 = p0;
    launch_frequency_shift(L, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

// ---- the gain envelope alone (EXTENSION; attacks.GainEnvelope, runtime.gain_envelope, tests) ----------------------------------
extern "C" int aware_gain_envelope(const float* in, const int* off, const int* len, int B, int max_len, const uint32_t* seeds,
                                   int step, int entry, int p_lo, int p_hi, float floor, float* out, float* gains, void* stream) {
    if (!in || !off || !len || !seeds || !out) return AWARE_E_BADARG;
    if (!ragged_args_ok(B, max_len) || step < 0 || entry < 0 || entry >= kMaxLoopAttacks) return AWARE_E_BADARG;
    if (p_lo < kEnvelopeMinPeriod || p_lo > p_hi || p_hi > kEnvelopeMaxPeriod || !(floor >= 0.f && floor < 1.f)) return AWARE_E_BADARG;
    GainLaunch L;
    L.in = in; L.out = out; L.gains = gains; L.off = off; L.len = len; L.B = B; L.max_len = max_len; L.seeds = seeds;
    L.step = step; L.entry = entry; L.p_lo = p_lo; L.p_hi = p_hi; L.floor = floor;
    launch_gain_envelope(L, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

// ---- the offset search's selection (EXTENSION; AWAREDetector.detect_batch(sync_search=n), tests) ---------------------------
extern "C" int aware_sync_select(const float* values, int B, int n, int L, float centre, float* out_values, int* out_index,
                                 float* out_conf, void* stream) {
    if (!values || !out_values || !out_index || !out_conf || values == out_values) return AWARE_E_BADARG;
    if (B < 1 || B > 65535 || n < 1 || n > 64 || L < 1 || L > 65536 || !std::isfinite(centre)) return AWARE_E_BADARG;
    launch_sync_select(values, B, n, L, centre, out_values, out_index, out_conf, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

// ---- the speed search's views (EXTENSION; AWAREDetector.detect_batch(speed_search=...), runtime.speed_views, tests) ---------
extern "C" int aware_speed_views(const float* in, const int* in_off, const int* in_len, int B, const int* m, int n_views,
                                 float* out, const int* out_off, int max_len, void* stream) {
    if (!in || !in_off || !in_len || !m || !out || !out_off || in == out) return AWARE_E_BADARG;
    if (!ragged_args_ok(B, max_len) || n_views < 1 || n_views > 63) return AWARE_E_BADARG;
    launch_speed_views(in, in_off, in_len, B, m, n_views, out, out_off, max_len, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

// ---- the shift search's views (EXTENSION; AWAREDetector.detect_batch(shift_search=...), runtime.shift_views, tests) ---------
extern "C" int aware_shift_views(const float* in, const int* in_off, const int* in_len, int B, const int* d, int n_views,
                                 float* out, const int* out_off, int max_len, void* stream) {
    if (!in || !in_off || !in_len || !d || !out || !out_off || in == out) return AWARE_E_BADARG;
    if (!ragged_args_ok(B, max_len) || n_views < 1 || n_views > 63) return AWARE_E_BADARG;
    launch_shift_views(in, in_off, in_len, B, d, n_views, out, out_off, max_len, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

// ---- scanning long recordings (EXTENSION; AWAREDetector.scan,runtime.scan_select, runtime.scan_segments, tests) ------------
// win_off is read on the host: B + 1 window offsets from 0, never falling, at least one window in all
static bool scan_offsets_ok(const int* win_off, int B) {
    if (win_off[0] != 0) return false;
    for (int b = 0; b < B; ++b)
        if (win_off[b + 1] < win_off[b]) return false;
    return win_off[B] >= 1;
}

extern "C" int aware_scan_select(const float* values, const int* win_off, int B, int n_sync, int L, float centre,
                                 float* win_conf, int* win_view, float* win_values, uint32_t* win_bits, void* stream) {
    if (!values || !win_off || !win_conf || !win_view || !win_values || !win_bits || values == win_values) return AWARE_E_BADARG;
    if (B < 1 || n_sync < 1 || n_sync > 64 || L < 1 || L > kScanMaxBits || !std::isfinite(centre)) return AWARE_E_BADARG;
    if (!scan_offsets_ok(win_off, B)) return AWARE_E_BADARG;
    launch_scan_select(values, win_off[B], n_sync, L, centre, win_conf, win_view, win_values, win_bits, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

extern "C" int aware_scan_segments(const float* win_conf, const int* win_view, const float* win_values, const uint32_t* win_bits,
                                   const int* win_off, const int* win_off_dev, int B, int L, float centre, float min_confidence,
                                   int max_flip, int max_segments, int* n_seg, int* seg_first, int* seg_last, int* seg_peak,
                                   int* seg_view, float* seg_conf, float* seg_values, void* stream) {
    if (!win_conf || !win_view || !win_values || !win_bits || !win_off || !win_off_dev || !n_seg || !seg_first || !seg_last ||
        !seg_peak || !seg_view || !seg_conf || !seg_values)
        return AWARE_E_BADARG;
    if (B < 1 || L < 1 || L > kScanMaxBits || !std::isfinite(centre) || !std::isfinite(min_confidence) || max_flip < 0 ||
        max_segments < 1)
        return AWARE_E_BADARG;
    if (!scan_offsets_ok(win_off, B)) return AWARE_E_BADARG;
    ScanSegments S;
    S.win_conf = win_conf; S.win_view = win_view; S.win_values = win_values; S.win_bits = win_bits; S.win_off = win_off_dev;
    S.B = B; S.L = L; S.max_flip = max_flip; S.max_segments = max_segments; S.centre = centre; S.min_conf = min_confidence;
    S.n_seg = n_seg; S.seg_first = seg_first; S.seg_last = seg_last; S.seg_peak = seg_peak; S.seg_view = seg_view;
    S.seg_conf = seg_conf; S.seg_values = seg_values;
    launch_scan_segments(S, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

// ---- coded payloads: the Viterbi decoder (EXTENSION; service.detect_message, AWAREDetector.scan, runtime.viterbi_decode, tests) --
extern "C" int aware_viterbi_decode(const float* values, int R, int L, float centre, int rate_n, int crc_bits, uint32_t* bits,
                                    float* metric, int* valid, int* corrected, void* stream) {
    if (!values || !bits || !metric || !valid || !corrected) return AWARE_E_BADARG;
    if (R < 1 || R > kViterbiMaxRows || L < 1 || L > kViterbiMaxBits || (rate_n != 2 && rate_n != 3)) return AWARE_E_BADARG;
    if ((crc_bits != 0 && crc_bits != 8 && crc_bits != 16) || !std::isfinite(centre)) return AWARE_E_BADARG;
    if (L / rate_n - 6 - crc_bits < 1) return AWARE_E_BADARG;
    launch_viterbi(values, R, L, centre, rate_n, crc_bits, bits, metric, valid, corrected, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

// ---- the phase vocoder's two kernels alone on a ragged spectrum (EXTENSION; runtime.pv_frames, runtime.pv_stretch, tests) -----
extern "C" int aware_pv_frames(const void* spec, const int* frame_off, int B, const int* mq, void* out, void* stream) {
    if (!spec || !frame_off || !mq || !out || spec == out || B < 1 || B > 65535) return AWARE_E_BADARG;
    PvLaunch L;
    L.spec = spec; L.out = out; L.draw.frame_off = frame_off; L.B = B; L.mq = mq;
    launch_pv_frames(L, 0, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}
extern "C" int aware_pv_frames_bwd(const void* spec, const void* grad_out, const int* frame_off, int B, const int* mq,
                                   void* grad_spec, void* stream) {
    if (!spec || !grad_out || !frame_off || !mq || !grad_spec || grad_out == grad_spec || B < 1 || B > 65535) return AWARE_E_BADARG;
    PvLaunch L;
    L.spec = spec; L.grad = grad_out; L.out = grad_spec; L.draw.frame_off = frame_off; L.B = B; L.mq = mq;
    launch_pv_frames(L, 1, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

extern "C" void aware_embed_destroy(aware_embed* e) {
    if (!e) return;

    if (e->gexec) (void)hipGraphExecDestroy(e->gexec);
    if (e->graph) (void)hipGraphDestroy(e->graph);
    if (e->gexecN) (void)hipGraphExecDestroy(e->gexecN);
    if (e->graphN) (void)hipGraphDestroy(e->graphN);
    if (e->cap) (void)hipStreamDestroy(e->cap);
    delete e;
}

extern "C" int aware_embed_conv_tile(const aware_embed* e, int backward, int layer) {
    if (!e || layer < 0 || layer >= e->det->n_layers) return AWARE_E_BADARG;
    // the conv kinds and tiles of a plan do not depend on its mel flags
    const DetPlan p = det_plan(e->det, e->b, e->cfg.conv_pipe, e->cfg.readout, false, false, false, e->cfg.conv_tile);
    if (backward) return layer <= p.top ? p.bwd_tile[layer] : 0;
    return layer < p.n_fwd ? p.fwd_tile[layer] : 0;
}

extern "C" void* aware_embed_buffer(aware_embed* e, int which) {
    if (!e) return nullptr;
    switch (which) {
        case 0: return e->loss;
        case 1: return e->best_loss;
        case 2: return e->db.pred;
        case 3: return e->coef;
        case 4: return e->best;
        case 5: return e->lo;
        case 6: return e->hi;
        case 7: return e->P;
        case 8: return e->step;
        case 9: return e->yraw;
        case 10: return e->mag;
        case 11: return e->opt.active ? e->opt.d_lr : nullptr;      // per-clip learning rate (double; ReduceLROnPlateau state)
        case 12:                                                    // the attacked signal of the last forward pass
            if (e->gc.n) return e->gc.z;
            return (e->la.n || e->mix_n) ? e->la.z : nullptr;
        case 13:                                                    // its impulse responses, f32 [B][8192]
            if (e->mix_n) return e->mix_rv >= 0 ? e->mix[e->mix_rv].h : nullptr;
            return (e->la.n && chain_has(e->la, AWARE_LOOP_REVERBERATION)) ? e->la.h : nullptr;
        case 14: return e->mix_n ? e->mix_choice : nullptr;         // a mixture's choices of the last forward pass, int [B]
        default: return nullptr;
    }
}

// ---- what one loop body needs on both routes ----
// the box of the coefficients: |c - c0| <= c0 * ratio, tolerance_db below the original magnitude
static float box_ratio(const aware_embed_config& cfg) { return (float)pow(10.0, -(double)cfg.tolerance_db / 20.0); }
// what det_forward_backward takes from the handle (the card route adds loss_add)
static DetGradCtx loop_grad_ctx(const aware_embed* e, int do_step) {
    DetGradCtx G;
    G.target = e->target; G.loss_kind = e->cfg.loss;
    G.loss = e->loss; G.d1 = e->d1; G.d2 = e->d2; G.gmag = e->gmag;
    G.step = do_step ? e->step : nullptr;               // the read-out kernel advances the step counter
    // aware_embed_gradient (do_step == 0) leaves the best-loss bookkeeping alone: the reference snapshots only
    // inside the optimiser loop (multibit_embedder.py:120-122)
    G.best_loss = do_step ? e->best_loss : nullptr;
    G.improved = do_step ? e->improved : nullptr;
    return G;
}
// the step of an optimiser / schedule set by aware_embed_set_optimizer, on the gradient the loop body left in gmag
static void own_optimizer_step(const aware_embed* e, hipStream_t st) {
    const aware_batch* b = e->b;
    const auto& o = e->opt;
    launch_opt_rows(o.kind, e->coef, e->gmag, e->mom, e->vel, e->c0, box_ratio(e->cfg), e->best, e->improved, b->d_frame_off, b->B,
                    b->NF, o.d_tab, e->cfg.num_iterations, e->step, o.plateau ? o.d_lr : nullptr, o.wd, o.hyp,
                    e->plan->dev.nband, e->plan->dev.stride, st);
    if (o.plateau) launch_plateau(e->loss, o.d_state, o.d_lr, b->B, o.factor, o.patience, o.threshold, o.min_lr, o.eps, st);
}

// ---- the general route (a general plan): the loop on the transforms of stft_any.hip and the band kernels of loop_any.hip ----
// the transforms on the synthesis' signal layout: clip b at out_off[b], hop (T_b - 1) samples, on both sides
static GenLaunch gen_loop_launch(const aware_embed* e) {
    GenLaunch L = gen_launch(e->plan, e->b);
    L.sig_off = e->b->d_out_off; L.sig_len = e->b->d_out_len;
    return L;
}
// [WaveformNormalizer, STFT, STFTDecomposer] on the whole spectrum: S0, then the band's magnitudes, unit phasors, box and
// optimiser state in one launch
static int gen_embed_begin(aware_embed* e, const float* audio, hipStream_t st) {
    const aware_batch* b = e->b;
    int rc = gen_stft(e->plan, b, audio, 1, e->S0, e->pmaxA, st);
    if (rc) return rc;
    BandBegin G;
    G.unit = e->U; G.coef = e->coef; G.lo = e->lo; G.hi = e->hi; G.mom = e->mom; G.vel = e->vel; G.best = e->best; G.c0 = e->c0;
    G.ratio = box_ratio(e->cfg);
    launch_band_mag(band_launch(e->plan, b), e->S0, e->mag, &G, true, st);
    LAUNCHCHK();
    return AWARE_OK;
}
// Assembler + ISTFT of `coef` into yraw, and the partial maxima of yraw
static int gen_synthesise(aware_embed* e, const float* coef, hipStream_t st) {
    const aware_batch* b = e->b;
    launch_band_assemble(band_launch(e->plan, b), coef, e->U, e->S0, st);
    LAUNCHCHK(); PROF(K_MISC);
    launch_gen_synthesis(gen_loop_launch(e), e->S0, e->yraw, 0, st);
    LAUNCHCHK(); PROF(K_SYNTH);
    launch_absmax_partials(e->yraw, b->d_out_off, b->d_out_len, e->pmaxY, b->pstride, b->B, b->max_len, st);
    LAUNCHCHK(); PROF(K_MISC);
    return AWARE_OK;
}
// the launches of the general route's chain (loop_any_chain.hip) on the loop's buffers
static GenChainLaunch gen_chain_launch(const aware_embed* e) {
    const aware_batch* b = e->b;
    const GenChainState& g = e->gc;
    GenChainLaunch C;
    C.sig_off = b->d_out_off; C.sig_len = b->d_out_len; C.pc_out = b->d_pc_out; C.B = b->B; C.pstride = b->pstride;
    C.pieces = g.pieces; C.step = e->step; C.seeds = g.seeds; C.n = g.n;
    for (int j = 0; j < g.n; ++j) {
        C.kind[j] = g.kind[j]; C.k[j] = g.k[j]; C.inv_snr[j] = g.inv_snr[j]; C.prob[j] = g.prob[j];
        C.p_lo[j] = g.p_lo[j]; C.p_hi[j] = g.p_hi[j]; C.floor[j] = g.floor[j];
    }
    C.yraw = e->yraw; C.pmaxY = e->pmaxY; C.psq = g.psq; C.z = g.z; C.pmaxZ = g.pmaxZ; C.a = e->y2;
    C.gy = e->gy; C.pdotA = g.pdotA; C.pdotX = g.pdotX;
    return C;
}
// one loop body of AWAREEmbedder._optimize (multibit_embedder.py:95-122), every stage its own launch, one chain
static int gen_embed_iteration(aware_embed* e, hipStream_t st, int do_step, float* grad_out) {
    const aware_batch* b = e->b;
    const aware_detector* d = e->det;
    const BandLaunch BL = band_launch(e->plan, b);
    const GenLaunch L = gen_loop_launch(e);
    // :99-103 scatter + Assembler + ISTFT, then the two normalisers (the post-process list ends with one, the pre-process
    // list starts with one), STFT and |.| on the band (:104 zeroes the rest)
    int rc = gen_synthesise(e, e->coef, st);
    if (rc) return rc;
    // attack-aware embedding (EXTENSION): x = N(N(yraw)), the chain's z, and a = N(N(z)) in y2, which the analysis reads
    const bool attacked = e->gc.n > 0;
    GenChainLaunch C;
    if (attacked) {
        C = gen_chain_launch(e);
        launch_gen_chain_forward(C, st);
    } else {
        launch_normalize(e->yraw, e->y1, b->d_out_off, b->d_out_len, e->pmaxY, b->d_pc_out, b->pstride, b->B, b->max_len, st);
        launch_absmax_partials(e->y1, b->d_out_off, b->d_out_len, e->pmaxY, b->pstride, b->B, b->max_len, st);
        launch_normalize(e->y1, e->y2, b->d_out_off, b->d_out_len, e->pmaxY, b->d_pc_out, b->pstride, b->B, b->max_len, st);
    }
    LAUNCHCHK(); PROF(K_MISC);
    launch_gen_analysis(L, e->y2, e->S2, 0, st);
    LAUNCHCHK(); PROF(K_ANALYSIS);
    launch_band_mag(BL, e->S2, e->mag, nullptr, false, st);
    LAUNCHCHK(); PROF(K_MISC);
    // :107 detector forward, :109 loss, :120-122 best tracking, :111 backward through the detector
    const DetPlan p = det_plan(d, b, e->cfg.conv_pipe, e->cfg.readout, false, false, false, e->cfg.conv_tile);
    rc = det_forward_backward(d, b, p, e->mag, e->db, loop_grad_ctx(e, do_step), st);
    if (rc) return rc;
    // backward through |.|, the STFT and its reflect padding, the two normalisers, the ISTFT and the assembler
    launch_band_mag_bwd(BL, e->S2, e->gmag, e->GS, st);
    LAUNCHCHK(); PROF(K_MISC);
    launch_gen_synthesis(L, e->GS, e->gy, 1, st);
    LAUNCHCHK(); PROF(K_SYNTH_ADJ);
    if (attacked) {
        // gy: dL/da -> dL/dyraw in place, at the step the forward pass drew at
        C.step_back = do_step ? 1 : 0;                  // the read-out kernel has advanced the counter
        launch_gen_chain_backward(C, st);
    } else {
        launch_normalize_bwd(e->y1, e->gy, e->gy1, b->d_out_off, b->d_out_len, b->B, st);
        launch_normalize_bwd(e->yraw, e->gy1, e->gy, b->d_out_off, b->d_out_len, b->B, st);
    }
    LAUNCHCHK(); PROF(K_MISC);
    launch_gen_analysis(L, e->gy, e->S2, 1, st);
    LAUNCHCHK(); PROF(K_ANALYSIS_ADJ);
    // :112-117 the step and the clamp: the card's NAdam inside the gradient kernel, any other optimiser / schedule in its
    // own launch on the gradient (left in gmag, which the backward above has consumed)
    const bool own_step = do_step && e->opt.active;
    BandStep S;
    S.coef = e->coef; S.mom = e->mom; S.vel = e->vel; S.best = e->best; S.lo = e->lo; S.hi = e->hi;
    S.improved = e->improved; S.sched = e->sched; S.sched_len = e->cfg.num_iterations + 1; S.step = e->step;
    memcpy(S.hyp, e->hyp, sizeof(S.hyp));
    launch_band_coef_grad(BL, e->S2, e->U, own_step ? e->gmag : grad_out, (do_step && !own_step) ? &S : nullptr, st);
    LAUNCHCHK(); PROF(K_MISC);
    if (own_step) {
        own_optimizer_step(e, st);
        LAUNCHCHK(); PROF(K_MISC);
    }
    return AWARE_OK;
}

static int embed_begin_state(aware_embed* e, const float* target, hipStream_t st);
extern "C" int aware_embed_begin(aware_embed* e, const float* audio, const float* target, void* stream) {
    if (!e || !audio || !target) return AWARE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const aware_batch* b = e->b;
    if (e->plan->general) {
        if (int rc = gen_embed_begin(e, audio, st)) return rc;
        return embed_begin_state(e, target, st);
    }
    // [WaveformNormalizer, STFT, STFTDecomposer] (multibit_embedder.py:143-147), band only
    launch_absmax_partials(audio, b->d_in_off, b->d_in_len, e->pmaxA, b->pstride, b->B, b->max_len, st);
    LAUNCHCHK();
    AnalysisLaunch L = analysis_launch(e->plan, b, audio, false);
    L.pmax = e->pmaxA;
    L.mag = e->mag; L.unit = e->P; L.unit_default = 1.f; L.polar_exact = 1;
    run_analysis(L, e->cfg.dsp_path, st);
    LAUNCHCHK();
    // constant out-of-band part of every synthesis: x/m - istft(band of the original)
    SynthLaunch S = synth_launch(e->plan, b);
    S.amp = e->mag; S.ph = e->P; S.out = e->gy; S.pstride = b->pstride;
    run_synth(S, e->cfg.dsp_path, st);
    LAUNCHCHK();
    launch_oob_residual(audio, b->d_in_off, e->pmaxA, b->d_pc_in, b->pstride, e->gy, b->d_frame_off, e->oob, b->B,
                        b->max_frames, st);
    LAUNCHCHK();
    launch_embed_prepare(e->mag, e->coef, e->lo, e->hi, e->mom, e->vel, e->best, e->c0, box_ratio(e->cfg),
                         (size_t)b->NF * e->plan->dev.stride, st);
    LAUNCHCHK();
    return embed_begin_state(e, target, st);
}
// the payload, the step counter, the best losses and a registry optimiser's per-clip state at the start of a run
static int embed_begin_state(aware_embed* e, const float* target, hipStream_t st) {
    const aware_batch* b = e->b;
    HIPCHK(hipMemcpyAsync(e->target, target, (size_t)b->B * e->det->nbits * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemsetAsync(e->step, 0, 4 * sizeof(int), st));
    // best_loss = +inf (0x7F800000)
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)e->best_loss, 0x7F800000, b->B, st));
    if (e->opt.active) {
        HIPCHK(hipMemcpyAsync(e->opt.d_lr, e->opt.lr_init.data(), (size_t)b->B * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(e->opt.d_state, e->opt.state_init.data(), (size_t)b->B * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    }
    e->steps_done = 0;
    return AWARE_OK;
}

// the loop side of a stage launch that serves entry `entry` of the chain
static LoopDraw loop_draw(const aware_embed* e, const LoopChainState& la, int step_back, int entry) {
    LoopDraw D;
    D.frame_off = e->b->d_frame_off; D.pstride = e->b->pstride; D.run_blocks = e->b->synth_run;
    D.step = e->step; D.step_back = step_back; D.seeds = la.seeds; D.entry = entry; D.prob = la.prob[entry];
    D.gate = la.gate;
    return D;
}
// a launch struct of the in -> out family (speed change, time stretch, pitch shift, sample deletion) for the splitting entry,
// or for the speed change of a stretch-then-speed pair
template <typename Launch>
static Launch stage_launch(const aware_embed* e, const LoopChainState& la, const float* in, float* out, int adjoint, int step_back,
                           bool of_pair = false) {
    Launch S;
    S.in = in; S.out = out; S.B = e->b->B; S.adjoint = adjoint;
    S.draw = loop_draw(e, la, step_back, of_pair ? la.pair_speed : la.split);
    return S;
}
static ResampleLaunch speed_launch(const aware_embed* e, const LoopChainState& la, const float* in, float* out, int adjoint, int step_back) {
    const bool of_pair = la.pair_speed >= 0;
    ResampleLaunch S = stage_launch<ResampleLaunch>(e, la, in, out, adjoint, step_back, of_pair);
    S.m_lo = of_pair ? la.lo2 : la.lo; S.m_hi = of_pair ? la.hi2 : la.hi;
    return S;
}
static DeleteLaunch delete_launch(const aware_embed* e, const LoopChainState& la, const float* in, float* out, int adjoint, int step_back) {
    DeleteLaunch S = stage_launch<DeleteLaunch>(e, la, in, out, adjoint, step_back);
    S.k_lo = la.lo; S.k_hi = la.hi; S.at = la.at;
    return S;
}
static ExcerptLaunch excerpt_launch(const aware_embed* e, const LoopChainState& la, const float* in, float* out, int adjoint, int step_back) {
    ExcerptLaunch S = stage_launch<ExcerptLaunch>(e, la, in, out, adjoint, step_back);
    S.l_lo = la.lo; S.l_hi = la.hi;
    return S;
}
static WarpLaunch warp_launch(const aware_embed* e, const LoopChainState& la, const float* in, float* out, int adjoint, int step_back) {
    WarpLaunch S = stage_launch<WarpLaunch>(e, la, in, out, adjoint, step_back);
    S.e_lo = la.lo; S.e_hi = la.hi; S.depth = la.depth;
    S.table_r = la.warpR; S.table_a = la.warpA; S.stride = la.kmax;
    return S;
}
static FilterLaunch filter_launch(const aware_embed* e, const LoopChainState& la, const float* in, float* out, int step_back) {
    FilterLaunch S = stage_launch<FilterLaunch>(e, la, in, out, 0, step_back);
    S.mask = la.mask; S.c_lo = la.lo; S.c_hi = la.hi; S.w_min = la.w_min;
    return S;
}
static ShiftLaunch shift_launch(const aware_embed* e, const LoopChainState& la, const float* in, float* out, int adjoint, int step_back) {
    ShiftLaunch S = stage_launch<ShiftLaunch>(e, la, in, out, adjoint, step_back);
    S.d_lo = la.lo; S.d_hi = la.hi;
    return S;
}
// the time stretch and the pitch shift: the window and one range of offsets
static ResampleLaunch ola_launch(const aware_embed* e, const LoopChainState& la, const float* in, float* out, int adjoint, int step_back) {
    ResampleLaunch S = stage_launch<ResampleLaunch>(e, la, in, out, adjoint, step_back);
    S.window = la.hann; S.m_lo = la.lo; S.m_hi = la.hi;
    return S;
}

// the phase vocoder's stage (kind 6).  Forward: STFT of u, the frames, iSTFT into `tmp`, u itself for the clips the entry leaves
// alone, the resampling of tmp into z.  The transforms are what aware_stft / aware_istft launch, on the loop's signal layout.
static PvLaunch pv_launch(const aware_embed* e, const LoopChainState& la, int step_back) {
    PvLaunch P;
    P.B = e->b->B; P.draw = loop_draw(e, la, step_back, la.split);
    P.q_lo = la.lo; P.q_hi = la.hi; P.m_lo = la.lo2; P.m_hi = la.hi2;
    return P;
}
static ResampleLaunch pv_speed_launch(const aware_embed* e, const LoopChainState& la, const float* in, float* out, int adjoint, int step_back) {
    ResampleLaunch S = stage_launch<ResampleLaunch>(e, la, in, out, adjoint, step_back);
    const bool has_m = la.lo2 <= la.hi2;
    S.m_lo = has_m ? la.lo2 : 0; S.m_hi = has_m ? la.hi2 : 0;      // stretch mode alone: m = 0, the identity
    S.coin = has_m && la.lo <= la.hi;
    return S;
}
static void pv_stage_forward(const aware_embed* e, const LoopChainState& la, float* tmp, hipStream_t st) {
    const aware_batch* b = e->b;
    AnalysisLaunch L = analysis_launch(e->plan, b, la.u, true);
    L.full = la.pvS; L.gate = la.gate;
    launch_analysis(L, st);
    PvLaunch P = pv_launch(e, la, 0);
    P.spec = la.pvS; P.out = la.pvY;
    launch_pv_frames(P, 0, st);
    SynthLaunch S = synth_launch(e->plan, b);
    S.full = la.pvY; S.out = tmp; S.pstride = b->pstride; S.gate = la.gate;
    launch_synth(S, st);
    launch_pv_idle(P, la.u, tmp, st);
    launch_speed_change(pv_speed_launch(e, la, tmp, la.z, 0, 0), st);
}
// The mirror: gz in u -> the resampling's adjoint into gy, the iSTFT's adjoint into the Y buffer, the frames' backward into the
// S buffer, the STFT's adjoint into gy, and gz itself for the clips the entry left alone
static void pv_stage_backward(const aware_embed* e, const LoopChainState& la, int step_back, hipStream_t st) {
    const aware_batch* b = e->b;
    launch_speed_change(pv_speed_launch(e, la, la.u, e->gy, 1, step_back), st);
    AnalysisLaunch L = analysis_launch(e->plan, b, e->gy, true);
    L.full = la.pvY; L.adjoint = 1; L.gate = la.gate;
    launch_analysis(L, st);
    PvLaunch P = pv_launch(e, la, step_back);
    P.spec = la.pvS; P.grad = la.pvY; P.out = la.pvS;
    launch_pv_frames(P, 1, st);
    SynthLaunch S = synth_launch(e->plan, b);
    S.full = la.pvS; S.out = e->gy; S.adjoint = 1; S.pstride = b->pstride; S.gate = la.gate;
    S.sig_off = b->d_out_off; S.sig_len = b->d_out_len;
    launch_synth(S, st);
    launch_pv_idle(P, la.u, e->gy, st);
}

static ConvolveLaunch reverb_launch(const aware_embed* e, const LoopChainState& la, const float* in, float* out, int adjoint) {
    ConvolveLaunch C;
    C.tables = la.tables; C.in = in; C.out = out; C.frame_off = e->b->d_frame_off; C.B = e->b->B; C.kmax = la.kmax;
    C.h = la.h; C.h_stride = kReverbMaxIr; C.nh = la.nh; C.parts = kReverbParts; C.adjoint = adjoint; C.skip_h = adjoint;
    C.hspec = la.hspec; C.xspec = la.xspec;
    C.gate = la.gate;
    return C;
}

// the launch struct of one chain's stage kernels: the chain of a plain handle, or chain c of a mixture behind its gate
static LoopAttackLaunch chain_stage_launch(const aware_embed* e, const LoopChainState& la) {
    const aware_batch* b = e->b;
    LoopAttackLaunch A;
    A.frame_off = b->d_frame_off; A.pcount = b->d_pc_syn; A.B = b->B; A.pstride = b->pstride; A.run_blocks = b->synth_run;
    A.step = e->step; A.seeds = la.seeds; A.n = la.n;
    for (int j = 0; j < la.n; ++j) { A.kind[j] = la.kind[j]; A.k[j] = la.k[j]; A.inv_snr[j] = la.inv_snr[j]; A.prob[j] = la.prob[j]; }
    for (int j = 0; j < la.n; ++j) { A.p_lo[j] = la.p_lo[j]; A.p_hi[j] = la.p_hi[j]; A.floor[j] = la.floor[j]; }
    A.yraw = e->yraw; A.pmaxY = e->pmaxY; A.psq = la.psq; A.z = la.z; A.pmaxZ = la.pmaxZ;
    // the idle rule (chain_idle): every chain with a splitting entry, and every chain that holds a gain envelope.  Chains of
    // noise and suppression alone keep the arithmetic of the loop before the rule existed, which recorded hashes pin.
    bool envelope = false;
    for (int j = 0; j < la.n; ++j) envelope = envelope || la.kind[j] == AWARE_LOOP_GAIN_ENVELOPE;
    if (chain_splits(la) || envelope) { A.idle_plain = 1; A.gpad_out = la.gpad0; }
    // inside a mixture the pads are shared between the chains: a chain of kinds 0/1 has no idle rule, and writes the zeros
    // its clips' pads hold on a plain handle
    if (la.gate.choice) A.gpad_out = la.gpad0;
    A.gate = la.gate;
    return A;
}
// the first entry behind the splitting stage
static int split_end(const LoopChainState& la) { return std::max(la.split, la.pair_speed) + 1; }
// the splitting stage, u -> z
static void split_forward(const aware_embed* e, const LoopChainState& la, hipStream_t st) {
    switch (la.split_kind) {
        case AWARE_LOOP_REVERBERATION: {
            ReverbIrLaunch R;
            R.seeds = la.seeds; R.step = e->step; R.entry = la.split; R.B = e->b->B; R.n_lo = la.lo; R.n_hi = la.hi;
            R.gain = la.gain; R.prob = la.prob[la.split]; R.h = la.h; R.h_stride = kReverbMaxIr; R.nh = la.nh; R.gate = la.gate;
            launch_reverb_ir(R, st);
            launch_convolve(reverb_launch(e, la, la.u, la.z, 0), st);
            break;
        }
        case AWARE_LOOP_SPEED_CHANGE: launch_speed_change(speed_launch(e, la, la.u, la.z, 0, 0), st); break;
        case AWARE_LOOP_TIME_STRETCH: {
            // the overlap-add, and the resampling of a speed change directly behind it through v
            const bool pair = la.pair_speed >= 0;
            launch_time_stretch(ola_launch(e, la, la.u, pair ? la.v : la.z, 0, 0), st);
            if (pair) launch_speed_change(speed_launch(e, la, la.v, la.z, 0, 0), st);
            break;
        }
        case AWARE_LOOP_PITCH_SHIFT: launch_pitch_shift(ola_launch(e, la, la.u, la.z, 0, 0), st); break;
        // gy is free until the synthesis adjoint writes it, and carries the vocoded signal to the resampling
        case AWARE_LOOP_PHASE_VOCODER: pv_stage_forward(e, la, e->gy, st); break;
        case AWARE_LOOP_BAND_FILTER: launch_band_filter(filter_launch(e, la, la.u, la.z, 0), st); break;
        case AWARE_LOOP_FREQUENCY_SHIFT: launch_frequency_shift(shift_launch(e, la, la.u, la.z, 0, 0), st); break;
        case AWARE_LOOP_EXCERPT: launch_excerpt_tile(excerpt_launch(e, la, la.u, la.z, 0, 0), st); break;
        // the table of the drawn rates first, then the resampling; the backward pass reads that table
        case AWARE_LOOP_TIME_WARP: launch_time_warp(warp_launch(e, la, la.u, la.z, 0, 0), st); break;
        default: launch_delete_samples(delete_launch(e, la, la.u, la.z, 0, 0), st); break;      // AWARE_LOOP_DELETE_SAMPLES
    }
}
// its mirror: the gradient behind the stage -> e->gy.  Every kind but the reverberation takes it from u (the forward pass is
// done with u) through its gather-form adjoint; the reverberation correlates gy in place with the same responses (their
// spectra are still there)
static void split_backward(const aware_embed* e, const LoopChainState& la, int step_back, hipStream_t st) {
    switch (la.split_kind) {
        case AWARE_LOOP_REVERBERATION: launch_convolve(reverb_launch(e, la, e->gy, e->gy, 1), st); break;
        case AWARE_LOOP_SPEED_CHANGE: launch_speed_change(speed_launch(e, la, la.u, e->gy, 1, step_back), st); break;
        case AWARE_LOOP_TIME_STRETCH: {
            const bool pair = la.pair_speed >= 0;
            if (pair) launch_speed_change(speed_launch(e, la, la.u, la.v, 1, step_back), st);
            launch_time_stretch(ola_launch(e, la, pair ? la.v : la.u, e->gy, 1, step_back), st);
            break;
        }
        case AWARE_LOOP_PITCH_SHIFT: launch_pitch_shift(ola_launch(e, la, la.u, e->gy, 1, step_back), st); break;
        case AWARE_LOOP_PHASE_VOCODER: pv_stage_backward(e, la, step_back, st); break;
        case AWARE_LOOP_BAND_FILTER: launch_band_filter(filter_launch(e, la, la.u, e->gy, step_back), st); break;      // its own adjoint
        case AWARE_LOOP_FREQUENCY_SHIFT: launch_frequency_shift(shift_launch(e, la, la.u, e->gy, 1, step_back), st); break;
        case AWARE_LOOP_EXCERPT: launch_excerpt_tile(excerpt_launch(e, la, la.u, e->gy, 1, step_back), st); break;
        case AWARE_LOOP_TIME_WARP: launch_time_warp(warp_launch(e, la, la.u, e->gy, 1, step_back), st); break;
        default: launch_delete_samples(delete_launch(e, la, la.u, e->gy, 1, step_back), st); break;
    }
}
// one chain's forward half: x = N(N(yraw)) -> z and its partial maxima
static void chain_forward(const aware_embed* e, const LoopChainState& la, const LoopAttackLaunch& A, hipStream_t st) {
    if (!chain_splits(la)) { launch_loop_attack_forward(A, st); return; }
    // the entries in front of the splitting entry on N(N(yraw)), its stage, the entries behind it
    launch_loop_attack_stage(A, 0, la.split, e->yraw, 1, la.u, nullptr, st);
    split_forward(e, la, st);
    launch_loop_attack_stage(A, split_end(la), la.n, la.z, 0, la.z, la.pmaxZ, st);
}
// its mirror: gy, dL/d N(N(z)) -> dL/dx, the partial sums against x and the reflect pads for the analysis adjoint
static void chain_backward(const aware_embed* e, const LoopChainState& la, LoopAttackLaunch& A, hipStream_t st) {
    if (!chain_splits(la)) { launch_loop_attack_backward(A, st); return; }
    // normalisers at z and the masks behind the stage (into u, unless the stage works on gy in place), the stage's adjoint
    // into gy, the masks in front of it and the partial sums against x
    A.gy_out = chain_has(la, AWARE_LOOP_REVERBERATION) ? nullptr : la.u;
    launch_loop_attack_stage_bwd(A, split_end(la), la.n, 1, 0, st);
    A.gy_out = nullptr;
    split_backward(e, la, A.step_back, st);
    launch_loop_attack_stage_bwd(A, 0, la.split, 0, 1, st);
}

// one loop body of AWAREEmbedder._optimize (multibit_embedder.py:95-122)
static int embed_iteration(aware_embed* e, hipStream_t st, int do_step, float* grad_out) {
    if (e->plan->general) return gen_embed_iteration(e, st, do_step, grad_out);
    const aware_batch* b = e->b;
    const aware_detector* d = e->det;
    // :99-103  scatter + Assembler + ISTFT  (out-of-band part is the constant `oob`)
    SynthLaunch S = synth_launch(e->plan, b);
    S.amp = e->coef; S.ph = e->P; S.out = e->yraw; S.add = e->oob; S.pmax = e->pmaxY; S.pstride = b->pstride;
    S.c0 = e->pl1 ? e->c0 : nullptr; S.pl1 = e->pl1;
    const int dsp = e->cfg.dsp_path;
    run_synth(S, dsp, st);
    LAUNCHCHK(); PROF(K_SYNTH);
    if (e->pl1) {
        launch_l1_reduce(e->pl1, b->d_pc_syn, b->pstride, b->d_frame_off, e->plan->dev.nband, e->cfg.l1_weight, e->l1term, b->B, st);
        LAUNCHCHK(); PROF(K_MISC);
    }
    // normalise x2 + STFT + |.| on the band (:104 zeroes the rest, so it is never computed)
    AnalysisLaunch L = analysis_launch(e->plan, b, e->yraw, true);
    L.pmax = e->pmaxY; L.double_norm = 1;
    // attack-aware embedding (EXTENSION): the chain turns the normalised synthesis into z; the analysis reads z
    const bool attacked = e->la.n > 0 || e->mix_n > 0;
    LoopAttackLaunch A, MA[kMaxLoopChains], AC;
    if (attacked) {
        const auto& la = e->la;
        if (e->mix_n) {
            // a mixture: the draw, every chain on the clips that drew it, the clips that drew none on the idle route of a
            // chain that splits (z = N(N(y)), maxima recorded as 1)
            LoopMixDrawLaunch D;
            D.seeds = la.seeds; D.step = e->step; D.B = b->B; D.n = e->mix_n; D.choice = e->mix_choice;
            for (int c = 0; c < e->mix_n; ++c) D.thr[c] = e->mix_thr[c];
            launch_loop_mix_draw(D, st);
            for (int c = 0; c < e->mix_n; ++c) {
                MA[c] = chain_stage_launch(e, e->mix[c]);
                chain_forward(e, e->mix[c], MA[c], st);
            }
            if (e->mix_thr[e->mix_n - 1] < 4294967296ull) {
                LoopChainState clean = la;
                clean.n = 0; clean.gate.choice = e->mix_choice; clean.gate.chain = -1;
                AC = chain_stage_launch(e, clean);
                AC.idle_plain = 1;
                launch_loop_attack_forward(AC, st);
            }
        } else {
            A = chain_stage_launch(e, la);
            chain_forward(e, la, A, st);
        }
        LAUNCHCHK(); PROF(K_MISC);
        L.sig = la.z; L.pmax = la.pmaxZ;
    }
    L.mag = e->mag; L.unit = e->U; L.unit_default = 0.f; L.write_pad = 0;
    // the mel projection as short runs of adjacent bins inside the streaming analysis kernel (no magnitude array), and its
    // backward as two taps per bin inside the synthesis adjoint (below): streaming DSP path and a filter bank of that form
    // (the tap forms serve 128 bands only: the synthesis adjoint reads dmel with a row stride of 128)
    const bool mel_taps = dsp == 0 && d->n_mels == 128 && d->melw && d->melm && stream_supported(e->plan->dev) && e->cfg.mel == 0;
    const bool mel_fold = mel_taps && d->melf_w && d->melf_s && d->n_mels == 128;
    if (mel_fold) { L.mel_out = e->db.xm; L.melf_w = d->melf_w; L.melf_s = d->melf_s; }
    run_analysis(L, dsp, st);
    LAUNCHCHK(); PROF(K_ANALYSIS);
    // :107 detector forward, :109 loss, :120-122 best tracking, :111 backward through the detector
    DetGradCtx G = loop_grad_ctx(e, do_step);
    G.loss_add = e->l1term;
    const DetPlan p = det_plan(d, b, e->cfg.conv_pipe, e->cfg.readout, false, mel_fold, mel_taps, e->cfg.conv_tile);
    int rc = det_forward_backward(d, b, p, e->mag, e->db, G, st);
    if (rc) return rc;
    // backward through |.|, STFT, reflect padding
    SynthLaunch SA = synth_launch(e->plan, b);
    SA.amp = e->gmag; SA.ph = e->U; SA.out = e->gy; SA.adjoint = 1; SA.yraw = e->yraw; SA.pmax_in = e->pmaxY;
    SA.pcount = b->d_pc_syn; SA.pdot = e->pdot; SA.pstride = b->pstride; SA.gpad = e->gpad;
    if (mel_taps) { SA.dmel = e->db.xm; SA.melw = d->melw; SA.melm = d->melm; }
    if (attacked) { SA.yraw = e->la.z; SA.pmax_in = e->la.pmaxZ; }
    run_synth(SA, dsp, st);
    LAUNCHCHK(); PROF(K_SYNTH_ADJ);
    if (attacked) {
        // gy: dL/d N(N(z)) -> dL/dx (normalisers at z, mask of the suppressions); the reflect-pad parts of the streaming
        // adjoint are folded in here, so the analysis adjoint below gets a block of zeros for them
        const bool streamed = dsp == 0 && stream_supported(e->plan->dev);
        auto arm = [&](LoopAttackLaunch& X) {
            X.step_back = do_step ? 1 : 0;              // the read-out kernel has advanced the counter
            X.gy = e->gy; X.gpad = streamed ? e->gpad : nullptr; X.pdot_in = e->pdot; X.pdot_out = e->la.pdot;
        };
        if (e->mix_n) {
            for (int c = 0; c < e->mix_n; ++c) { arm(MA[c]); chain_backward(e, e->mix[c], MA[c], st); }
            if (e->mix_thr[e->mix_n - 1] < 4294967296ull) { arm(AC); launch_loop_attack_backward(AC, st); }
        } else {
            arm(A);
            chain_backward(e, e->la, A, st);
        }
        LAUNCHCHK(); PROF(K_MISC);
    }
    // backward through the normalisers, ISTFT and the assembler; :112-117 NAdam + clamp
    AnalysisLaunch LA = analysis_launch(e->plan, b, e->gy, true);
    LA.pmax = e->pmaxY; LA.adjoint = 1; LA.yraw = e->yraw; LA.pdot = e->pdot; LA.phasor = e->P;
    LA.coef = e->coef; LA.mom = e->mom; LA.vel = e->vel; LA.lo = e->lo; LA.hi = e->hi; LA.best = e->best;
    LA.improved = e->improved; LA.sched = e->sched; LA.sched_len = e->cfg.num_iterations + 1; LA.step = e->step;
    // (an optimiser / schedule set by aware_embed_set_optimizer steps in its own launch below: the adjoint then only
    //  delivers the gradient, into gmag -- consumed by the synthesis adjoint by now)
    const bool own_step = do_step && e->opt.active;
    LA.grad_out = own_step ? e->gmag : grad_out; LA.do_step = own_step ? 0 : do_step;
    memcpy(LA.hyp, e->hyp, sizeof(LA.hyp));
    LA.gpad = e->gpad; LA.c0 = e->c0; LA.box_ratio = box_ratio(e->cfg);
    LA.l1_weight = e->pl1 ? e->cfg.l1_weight : 0.f;
    if (attacked) { LA.pdot = e->la.pdot; LA.gpad = e->la.gpad0; }
    run_analysis(LA, dsp, st);
    LAUNCHCHK(); PROF(K_ANALYSIS_ADJ);
    if (own_step) {
        own_optimizer_step(e, st);
        LAUNCHCHK(); PROF(K_MISC);
    }
    return AWARE_OK;
}

extern "C" int aware_embed_iterate(aware_embed* e, int n_iters, void* stream) {
    if (!e || n_iters < 0) return AWARE_E_BADARG;
    // the NAdam schedule table holds cfg.num_iterations steps (the reference's loop runs exactly that many,
    // multibit_embedder.py:95): more than that since aware_embed_begin is a caller error
    if (e->steps_done + n_iters > e->cfg.num_iterations) return AWARE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (n_iters > 0) e->la.locked = true;
    if (!e->cfg.use_graph) {
        for (int i = 0; i < n_iters; ++i) {
            int rc = embed_iteration(e, st, 1, nullptr);
            if (rc) return rc;
            ++e->steps_done;
        }
        return AWARE_OK;
    }
    // Two graphs: one loop body, and kGraphIters loop bodies (amortises the replay floor).  The
    // caller's stream may be the legacy default stream, which cannot be captured: record on a
    // private stream, replay on the caller's.  All kernel arguments are iteration-invariant
    // (the optimiser step index lives in device memory), so one recording serves every replay.
    constexpr int kGraphIters = 16;
    if (!e->gexec) {
        if (!e->cap) HIPCHK(hipStreamCreateWithFlags(&e->cap, hipStreamNonBlocking));
        for (int which = 0; which < 2; ++which) {
            HIPCHK(hipStreamBeginCapture(e->cap, hipStreamCaptureModeThreadLocal));
            int rc = AWARE_OK;
            for (int i = 0; i < (which ? kGraphIters : 1) && rc == AWARE_OK; ++i) rc = embed_iteration(e, e->cap, 1, nullptr);
            hipGraph_t g = nullptr;
            hipError_t ce = hipStreamEndCapture(e->cap, &g);
            hipGraphExec_t ge = nullptr;
            if (rc == AWARE_OK && ce == hipSuccess) ce = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
            if (rc != AWARE_OK || ce != hipSuccess) {
                // no half-recorded state: drop whatever exists (both graphs) so that a later call records again
                if (ge) (void)hipGraphExecDestroy(ge);
                if (g) (void)hipGraphDestroy(g);
                if (e->gexec) { (void)hipGraphExecDestroy(e->gexec); e->gexec = nullptr; }
                if (e->graph) { (void)hipGraphDestroy(e->graph); e->graph = nullptr; }
                if (rc != AWARE_OK) return rc;
                HIPCHK(ce);
            }
            if (which) { e->graphN = g; e->gexecN = ge; } else { e->graph = g; e->gexec = ge; }
        }
    }
    int left = n_iters;
    for (; left >= kGraphIters; left -= kGraphIters) { HIPCHK(hipGraphLaunch(e->gexecN, st)); e->steps_done += kGraphIters; }
    for (; left > 0; --left) { HIPCHK(hipGraphLaunch(e->gexec, st)); ++e->steps_done; }
    return AWARE_OK;
}

extern "C" int aware_embed_profile(aware_embed* e, int n_iters, int max_entries, float* ms_out, int* kind_out,
                                   void* stream) {
    if (!e || !ms_out || !kind_out || n_iters < 1) return AWARE_E_BADARG;
    if (e->steps_done + n_iters > e->cfg.num_iterations) return AWARE_E_BADARG;      // as aware_embed_iterate
    hipStream_t st = (hipStream_t)stream;
    LaunchProfiler p;
    p.st = st;
    g_prof = &p;
    prof_mark(-1);
    int rc = AWARE_OK;
    for (int i = 0; i < n_iters && rc == AWARE_OK; ++i) { rc = embed_iteration(e, st, 1, nullptr); if (rc == AWARE_OK) ++e->steps_done; }
    g_prof = nullptr;
    hipError_t se = hipStreamSynchronize(st);
    int n = 0;
    for (size_t i = 1; i < p.ev.size(); ++i) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, p.ev[i - 1], p.ev[i]);
        if (n < max_entries) { ms_out[n] = ms; kind_out[n] = p.kind[i]; ++n; }
    }
    for (auto& ev : p.ev) (void)hipEventDestroy(ev);
    if (rc) return rc;
    HIPCHK(se);
    return n;      // number of entries written (>= 0)
}

extern "C" int aware_embed_gradient(aware_embed* e, float* grad, void* stream) {
    if (!e || !grad) return AWARE_E_BADARG;
    return embed_iteration(e, (hipStream_t)stream, 0, grad);
}

extern "C" int aware_embed_finish(aware_embed* e, const float* rescale, float* out, void* stream) {
    if (!e || !out) return AWARE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const aware_batch* b = e->b;
    if (e->plan->general) {
        // the best coefficients through the assembler and the ISTFT, one normaliser, the caller's rescale
        if (int rc = gen_synthesise(e, e->best, st)) return rc;
        launch_rescale_normalize(e->yraw, out, b->d_out_off, b->d_out_len, e->pmaxY, b->d_pc_out, b->pstride, rescale, b->B,
                                 b->max_len, st);
        LAUNCHCHK();
        return AWARE_OK;
    }
    SynthLaunch S = synth_launch(e->plan, b);
    S.amp = e->best; S.ph = e->P; S.out = e->yraw; S.add = e->oob; S.pmax = e->pmaxY; S.pstride = b->pstride;
    run_synth(S, e->cfg.dsp_path, st);
    LAUNCHCHK();
    launch_finish(e->yraw, b->d_frame_off, e->pmaxY, b->d_pc_syn, b->pstride, rescale, out, b->d_out_off, b->B,
                  b->max_frames, st);
    LAUNCHCHK();
    return AWARE_OK;
}

// ---------------------------------------------------------------------------------------------
extern "C" int aware_pcm_quantize(const float* in, float* out, const int* off, const int* len, int B, int max_len,
                                  int bits, void* scratch, void* stream) {
    if (!in || !out || !off || !len || !scratch || B < 1) return AWARE_E_BADARG;
    float q, lo, hi;
    switch (bits) {   // scripts/attacks.py:52-67 (the "12-bit" branch really is 13-bit)
        case 8: q = 127.f; lo = -128.f; hi = 127.f; break;
        case 12: q = 4095.f; lo = -4096.f; hi = 4095.f; break;
        case 16: q = 32767.f; lo = -32768.f; hi = 32767.f; break;
        case 24: q = 8388607.f; lo = -8388608.f; hi = 8388607.f; break;
        default: return AWARE_E_BADARG;   // reference raises ValueError
    }
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* pmax; int* pcount; int ps;
    int rc = absmax_into_scratch(in, off, len, B, max_len, scratch, &pmax, &pcount, &ps, st);
    if (rc) return rc;
    launch_pcm_quantize(in, out, off, len, pmax, pcount, ps, q, lo, hi, B, max_len, st);
    LAUNCHCHK();
    return AWARE_OK;
}

// shared by the max-abs normalising entry points: partial maxima + counts in `scratch`
static int absmax_into_scratch(const float* in, const int* off, const int* len, int B, int max_len, void* scratch,
                               unsigned long long** pmax_out, int** pcount_out, int* ps_out, hipStream_t st) {
    const int ps = (max_len + 4095) / 4096;
    unsigned long long* pmax = (unsigned long long*)scratch;
    int* pcount = (int*)(pmax + (size_t)B * ps);
    HIPCHK(hipMemsetAsync(pmax, 0, (size_t)B * ps * sizeof(unsigned long long), st));
    launch_absmax_partials(in, off, len, pmax, ps, B, max_len, st);
    LAUNCHCHK();
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)pcount, ps, B, st));
    *pmax_out = pmax; *pcount_out = pcount; *ps_out = ps;
    return AWARE_OK;
}

extern "C" int aware_waveform_normalize(const float* in, float* out, const int* off, const int* len, int B,
                                        int max_len, void* scratch, void* stream) {
    if (!in || !out || !off || !len || !scratch || B < 1) return AWARE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* pmax; int* pcount; int ps;
    int rc = absmax_into_scratch(in, off, len, B, max_len, scratch, &pmax, &pcount, &ps, st);
    if (rc) return rc;
    launch_normalize(in, out, off, len, pmax, pcount, ps, B, max_len, st);
    LAUNCHCHK();
    return AWARE_OK;
}

extern "C" int aware_upfirdn(const float* in, const int* in_off, const int* in_len, float* out, const int* out_off,
                             const int* out_len, int B, int max_out, const float* h, int nh, int up, int down,
                             int half_len, void* stream) {
    if (!in || !out || !h || B < 1 || nh < 1 || up < 1 || down < 1 || half_len < 0) return AWARE_E_BADARG;
    launch_upfirdn(in, in_off, in_len, out, out_off, out_len, h, nh, up, down, half_len, B, max_out,
                   (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

extern "C" int aware_iir(const float* in, const int* off, const int* len, int B, int max_len, void* out, int out_f64,
                         const double* b, const double* a, const double* zi, int ncoef, int filtfilt, void* scratch,
                         void* stream) {
    if (!in || !out || !b || !a || B < 1 || ncoef < 2 || ncoef > 12) return AWARE_E_BADARG;
    if (filtfilt && (!zi || !scratch)) return AWARE_E_BADARG;
    launch_iir_full(in, off, len, out, out_f64, b, a, zi, ncoef, filtfilt ? 1 : 0, (double*)scratch,
                    max_len + 6 * ncoef, B, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

extern "C" int aware_decimate_interp(const float* in, const int* off, const int* len, int B, int max_len, int factor,
                                     double* out, void* stream) {
    if (!in || !off || !len || !out || B < 1 || factor < 2) return AWARE_E_BADARG;
    launch_decimate_interp(in, off, len, out, factor, B, max_len, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

extern "C" int aware_segment_cut(const float* in, const int* in_off, float* out, const int* out_off,
                                 const int* out_len, const int* cut_start, const int* cut_len, int zero_fill, int B,
                                 int max_len, void* stream) {
    if (!in || !out || B < 1) return AWARE_E_BADARG;
    launch_segment_copy(in, in_off, out, out_off, out_len, cut_start, cut_len, zero_fill, B, max_len,
                        (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

extern "C" int aware_gaussian_noise(const float* in, float* out, const int* off, const int* len, int B, int max_len,
                                    const uint32_t* seeds, float snr_db, void* scratch, void* stream) {
    if (!in || !out || !seeds || !scratch || B < 1) return AWARE_E_BADARG;
    launch_gaussian_noise_full(in, out, off, len, seeds, (double*)scratch, snr_db, B, max_len, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

extern "C" int aware_snr(const float* output, const int* out_offsets, const float* target, const int* tgt_offsets,
                         const int* lengths, int B, double* snr_db, void* stream) {
    if (!output || !out_offsets || !target || !tgt_offsets || !lengths || !snr_db || B < 1) return AWARE_E_BADARG;
    launch_snr(output, out_offsets, target, tgt_offsets, lengths, snr_db, B, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

// ---- STOI (stoi_kernels.hip) -------------------------------------------------------------------------------------------
struct aware_stoi_plan {
    void* mem = nullptr;
    StoiTables tab;
    int band_lo[kStoiRow] = {0}, band_hi[kStoiRow] = {0};
};

// third-octave band k: the bins of a 512-point spectrum at 10 kHz closest to 150 * 2^((2k -+ 1)/6) Hz, [lo, hi)
// (metrics/audio.py::_third_octave_matrix: argmin of the squared distance, the first bin on a tie)
static void stoi_band_edges(int* lo, int* hi) {
    const int nfft = 2 * kStoiFrame, nbin = nfft / 2 + 1;
    const double fs = 10000.0;
    auto nearest = [&](double f) {
        int best = 0;
        double bd = INFINITY;
        for (int i = 0; i < nbin; ++i) {
            const double d = (fs * i / nfft - f) * (fs * i / nfft - f);
            if (d < bd) { bd = d; best = i; }
        }
        return best;
    };
    for (int k = 0; k < kStoiBands; ++k) {
        lo[k] = nearest(150.0 * pow(2.0, (2 * k - 1) / 6.0));
        hi[k] = nearest(150.0 * pow(2.0, (2 * k + 1) / 6.0));
    }
    for (int k = kStoiBands; k < kStoiRow; ++k) lo[k] = hi[k] = 0;
}

extern "C" int aware_stoi_create(aware_stoi_plan** out) {
    if (!out) return AWARE_E_BADARG;
    const double PI = 3.14159265358979323846;
    const int M = kStoiFrame, N = 2 * M;
    Building<aware_stoi_plan, aware_stoi_destroy> p(new aware_stoi_plan());
    stoi_band_edges(p->band_lo, p->band_hi);
    // device image: th [M/2] cf, twN [M + 1 -> M + 2] cf, window [256] f32, bands [32] int
    std::vector<float> h(M + 2 * (M + 2) + kStoiFrame + 2 * kStoiRow, 0.f);
    float* th = h.data();
    float* twN = th + M;
    float* win = twN + 2 * (M + 2);
    int* bands = reinterpret_cast<int*>(win + kStoiFrame);
    for (int j = 0; j < M / 2; ++j) {
        th[2 * j] = (float)cos(2 * PI * j / M);
        th[2 * j + 1] = (float)-sin(2 * PI * j / M);
    }
    for (int k = 0; k <= M; ++k) {
        twN[2 * k] = (float)cos(2 * PI * k / N);
        twN[2 * k + 1] = (float)-sin(2 * PI * k / N);
    }
    twN[0] = 1.f; twN[1] = 0.f;
    twN[M] = 0.f; twN[M + 1] = -1.f;
    twN[2 * M] = -1.f; twN[2 * M + 1] = 0.f;
    for (int i = 0; i < kStoiFrame; ++i)                   // np.hanning(258)[1:-1]
        win[i] = (float)(0.5 - 0.5 * cos(2 * PI * (i + 1) / (kStoiFrame + 1)));
    for (int k = 0; k < kStoiRow; ++k) { bands[k] = p->band_lo[k]; bands[kStoiRow + k] = p->band_hi[k]; }
    if (hipMalloc(&p->mem, h.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(p->mem, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        g_last_err = "aware_stoi_create: device tables";
        return AWARE_E_HIP;
    }
    float* d = (float*)p->mem;
    p->tab.th = (const cf*)d;
    p->tab.twN = (const cf*)(d + M);
    p->tab.window = d + M + 2 * (M + 2);
    p->tab.bands = (const int*)(d + M + 2 * (M + 2) + kStoiFrame);
    *out = p.release();
    return AWARE_OK;
}

extern "C" void aware_stoi_destroy(aware_stoi_plan* p) {
    if (!p) return;
    if (p->mem) (void)hipFree(p->mem);
    delete p;
}

extern "C" int aware_stoi_band_edges(const aware_stoi_plan* p, int* lo, int* hi) {
    if (!lo || !hi) return AWARE_E_BADARG;
    if (p) {
        memcpy(lo, p->band_lo, kStoiBands * sizeof(int));
        memcpy(hi, p->band_hi, kStoiBands * sizeof(int));
    } else {
        int l[kStoiRow], h[kStoiRow];
        stoi_band_edges(l, h);
        memcpy(lo, l, kStoiBands * sizeof(int));
        memcpy(hi, h, kStoiBands * sizeof(int));
    }
    return AWARE_OK;
}

extern "C" int aware_stoi_frames(int n) { return n < 0 ? AWARE_E_BADARG : stoi_frames(n); }

// rows of the per-frame arrays: every clip's first-stage frames, all kept (frames(n) <= n / 128)
static size_t stoi_total_frames(int B, int max_len, long long total_len) {
    const size_t by_max = (size_t)B * (size_t)stoi_frames(max_len), by_total = (size_t)(total_len / kStoiHop);
    return std::max<size_t>(1, std::min(by_max, by_total));
}
struct StoiCarve {
    size_t energy, kept, kcount, fbase, xt, yt, partial, total;
};
static StoiCarve stoi_carve(int B, int max_len, long long total_len) {
    const size_t TF = stoi_total_frames(B, max_len, total_len);
    StoiCarve c;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
    c.energy = take(TF * sizeof(double));
    c.kept = take(TF * sizeof(int));
    c.kcount = take((size_t)B * sizeof(int));
    c.fbase = take((size_t)B * sizeof(int));
    c.xt = take(TF * kStoiRow * sizeof(float));
    c.yt = take(TF * kStoiRow * sizeof(float));
    c.partial = take((size_t)B * stoi_partials(max_len) * sizeof(double));
    c.total = o;
    return c;
}

extern "C" size_t aware_stoi_workspace_bytes(int B, int max_len, long long total_len) {
    if (B < 1 || max_len < 0 || total_len < 0) return 0;
    return stoi_carve(B, max_len, total_len).total;
}

extern "C" int aware_stoi(const aware_stoi_plan* plan, const float* clean, const int* clean_off, const float* proc,
                          const int* proc_off, const int* n, int B, int max_len, long long total_len, double* out,
                          int* kept_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!plan || !clean || !clean_off || !proc || !proc_off || !n || !out || !workspace) return AWARE_E_BADARG;
    if (B < 1 || B > 65535 || max_len < 0 || total_len < max_len || total_len > (long long)B * max_len) return AWARE_E_BADARG;
    const StoiCarve c = stoi_carve(B, max_len, total_len);
    if (workspace_bytes < c.total) return AWARE_E_WORKSPACE;
    char* ws = (char*)workspace;
    StoiLaunch L;
    L.tab = plan->tab;
    L.clean = clean; L.clean_off = clean_off;
    L.proc = proc; L.proc_off = proc_off;
    L.n = n;
    L.B = B;
    L.max_frames = stoi_frames(max_len);
    L.max_partials = stoi_partials(max_len);
    L.energy = (double*)(ws + c.energy);
    L.kept = (int*)(ws + c.kept);
    L.kcount = (int*)(ws + c.kcount);
    L.fbase = (int*)(ws + c.fbase);
    L.xt = (float*)(ws + c.xt);
    L.yt = (float*)(ws + c.yt);
    L.partial = (double*)(ws + c.partial);
    L.out = out;
    L.kept_out = kept_out;
    launch_stoi(L, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

extern "C" int aware_phase_vocoder(const void* spec_in, const int* frame_off_in, void* spec_out, const int* frame_off_out,
                                   int B, double rate, void* stream) {
    if (!spec_in || !frame_off_in || !spec_out || !frame_off_out || B < 1 || !(rate > 0.0)) return AWARE_E_BADARG;
    launch_phase_vocoder(spec_in, frame_off_in, spec_out, frame_off_out, rate, B, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

extern "C" int aware_spectral_quantize(void* spec, int n_frames, float step_db, float floor_db, void* stream) {
    if (!spec || n_frames < 1 || !(step_db > 0.f)) return AWARE_E_BADARG;
    launch_spectral_quantize(spec, n_frames, step_db, floor_db, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

extern "C" int aware_spectral_quantize_bwd(const void* spec_in, const void* grad_out, void* grad_in, int n_frames, float step_db,
                                           float floor_db, void* stream) {
    if (!spec_in || !grad_out || !grad_in || n_frames < 1 || !(step_db > 0.f)) return AWARE_E_BADARG;
    launch_spectral_quantize_bwd(spec_in, grad_out, grad_in, n_frames, step_db, floor_db, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

extern "C" int aware_gemm_nt_variant(const float* A, int lda, const float* Bt, int ldb, const float* bias, float* C,
                                     int ldc, int M, int N, int K, int variant, void* stream) {
    if (!A || !Bt || !C || M < 1 || N < 1 || K < 4 || (K & 3) || (lda & 3) || (ldb & 3) || variant < 0 || variant > 16)
        return AWARE_E_BADARG;
    launch_gemm_nt_variant(A, lda, Bt, ldb, bias, C, ldc, M, N, K, variant, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}

// clip-aligned GEMM alone (tests / roofline): mode 0 = f32 MFMA kernel on Bt, mode 1 = bf16 three-way split kernel on Bpk
extern "C" size_t aware_x3_packed_bytes(int N, int K) { return (N > 0 && K > 0 && N % 16 == 0) ? x3_packed_bytes(N, K) : 0; }
extern "C" int aware_x3_pack(const float* host_wt, int N, int K, void* host_out) {
    if (!host_wt || !host_out || N < 16 || N % 16 || K < 1) return AWARE_E_BADARG;
    x3_pack(host_wt, N, K, (uint16_t*)host_out);
    return AWARE_OK;
}
extern "C" int aware_gemm_clip(const float* A, int lda, const float* Bt, int ldb, const void* Bpk, const float* bias, float* C,
                               int ldc, int B, int Tp, int N, int K, int epi, float* rstd_io, const float* act, int mode,
                               void* stream) {
    if (!A || !C || B < 1 || Tp < 1 || Tp > 128 || N < 1 || K < 4 || (K & 3) || (lda & 3) || epi < 0 || epi > 2) return AWARE_E_BADARG;
    if (epi != 0 && !rstd_io) return AWARE_E_BADARG;
    if (epi == 2 && !act) return AWARE_E_BADARG;
    const int nwm = (Tp + 31) / 32;
    if (mode == 1) {
        if (!Bpk || !gemm_clip_x3_supported(nwm, N, K, lda)) return AWARE_E_BADARG;
        launch_gemm_clip_x3(A, lda, Bpk, bias, C, ldc, B, nwm, Tp, N, K, epi, rstd_io, act, (hipStream_t)stream);
    } else {
        if (!Bt || (ldb & 3)) return AWARE_E_BADARG;
        launch_gemm_clip(A, lda, Bt, ldb, bias, C, ldc, B, nwm, Tp, N, K, epi, rstd_io, act, (hipStream_t)stream);
    }
    LAUNCHCHK();
    return AWARE_OK;
}

// the forward conv block whose epilogue also emits the split-K partials of the NEXT (skinny, CL <= 48 channels) conv:
// the kernel the embed loop runs for block 2 (X3_FWD_LAST).  Test / roofline entry; always the throughput kernel.
extern "C" int aware_gemm_clip_last(const float* A, int lda, const void* Bpk, const float* bias, float* C, int ldc, int B, int Tp,
                                    int N, int K, float* rstd_out, const void* lastpk, float* zpart, int CL, void* stream) {
    if (!A || !Bpk || !C || !rstd_out || !lastpk || !zpart || B < 1 || Tp < 1 || Tp > 128 || CL < 2 || CL > 48) return AWARE_E_BADARG;
    const int nwm = (Tp + 31) / 32;
    if (!gemm_clip_x3_supported(nwm, N, K, lda)) return AWARE_E_BADARG;
    launch_gemm_clip_x3(A, lda, Bpk, bias, C, ldc, B, nwm, Tp, N, K, 1, rstd_out, nullptr, (hipStream_t)stream, lastpk, zpart, CL);
    LAUNCHCHK();
    return AWARE_OK;
}

// the same block(s) on the f16 two-term kernel (gemm_h2.hip), test / roofline entry: packs Bt (device, [N][K]) and computes
// the per-clip maxima of A into `workspace` first.  epi 0..2 as aware_gemm_clip; lastpk / zpart / CL (epi 1 only, may be
// null / 0) as aware_gemm_clip_last.
extern "C" size_t aware_gemm_clip_h2_workspace_bytes(int B, int N, int K) {
    return (B > 0 && N > 0 && K > 0) ? h2_packed_bytes(N, K) + (size_t)B * 64 * sizeof(float) * 2 + 1024 : 0;
}
extern "C" int aware_gemm_clip_h2(const float* A, int lda, const float* Bt, int ldb, const float* bias, float* C, int ldc, int B,
                                  int Tp, int N, int K, int epi, float* rstd_io, const float* act, const void* lastpk, float* zpart,
                                  int CL, float* amax_out, void* workspace, size_t workspace_bytes, void* stream) {
    return aware_gemm_clip_h2_tile(A, lda, Bt, ldb, bias, C, ldc, B, Tp, N, K, epi, rstd_io, act, lastpk, zpart, CL, amax_out,
                                   workspace, workspace_bytes, 0, stream);
}
// tile 0: the 128-column form (what the entry above runs; the automatic choice belongs to a session's plan), 1: the same,
// 2: the wide form (AWARE_E_UNSUPPORTED where it cannot run: more than 96 rows per clip, N no multiple of 256)
extern "C" int aware_gemm_clip_h2_tile(const float* A, int lda, const float* Bt, int ldb, const float* bias, float* C, int ldc,
                                       int B, int Tp, int N, int K, int epi, float* rstd_io, const float* act, const void* lastpk,
                                       float* zpart, int CL, float* amax_out, void* workspace, size_t workspace_bytes, int tile,
                                       void* stream) {
    if (tile < 0 || tile > 2) return AWARE_E_BADARG;
    if (!A || !Bt || !C || !workspace || B < 1 || Tp < 1 || Tp > 128 || epi < 0 || epi > 2 || (ldb & 3)) return AWARE_E_BADARG;
    if (epi != 0 && !rstd_io) return AWARE_E_BADARG;
    if (epi == 2 && !act) return AWARE_E_BADARG;
    const int nwm = (Tp + 31) / 32;
    if (!gemm_clip_h2_supported(nwm, N, K, lda) || N % 16) return AWARE_E_BADARG;
    if (tile == 2 && !gemm_clip_h2_wide_supported(nwm, N, K, lda)) return AWARE_E_UNSUPPORTED;
    if (workspace_bytes < aware_gemm_clip_h2_workspace_bytes(B, N, K)) return AWARE_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    Carver c(workspace, workspace_bytes);
    void* pk = c.take<char>(h2_packed_bytes(N, K));
    float* amax = c.take<float>((size_t)B * 64);
    launch_h2_pack(Bt, ldb, N, K, pk, st);
    launch_clip_amax(A, lda, K, 32 * nwm, B, amax, st);
    launch_gemm_clip_h2(A, lda, pk, amax, amax_out, bias, C, ldc, B, nwm, Tp, N, K, epi, rstd_io, act, st,
                        (epi == 1 && lastpk && zpart) ? lastpk : nullptr, zpart, CL, tile == 2 ? 2 : 1);
    LAUNCHCHK();
    return AWARE_OK;
}
// the form aware_gemm_clip_h2_tile runs for these arguments (the launcher's own decision): 1 = 128-column, 2 = wide with the
// accumulator-layout epilogue, 3 = wide with the row-major epilogue; AWARE_E_* as the entry above would return
extern "C" int aware_gemm_clip_h2_form(const float* C, int ldc, const float* act, int Tp, int N, int K, int lda, int epi, int last,
                                       int tile) {
    if (tile < 0 || tile > 2 || !C || Tp < 1 || Tp > 128 || epi < 0 || epi > 2) return AWARE_E_BADARG;
    const int nwm = (Tp + 31) / 32;
    if (!gemm_clip_h2_supported(nwm, N, K, lda) || N % 16) return AWARE_E_BADARG;
    if (tile == 2 && !gemm_clip_h2_wide_supported(nwm, N, K, lda)) return AWARE_E_UNSUPPORTED;
    return gemm_clip_h2_form(tile == 2 ? 2 : 1, nwm, epi, last != 0, C, ldc, act);
}

extern "C" int aware_gemm_nt(const float* A, int lda, const float* Bt, int ldb, const float* bias, float* C, int ldc,
                             int M, int N, int K, void* stream) {
    if (!A || !Bt || !C || M < 1 || N < 1 || K < 4 || (K & 3) || (lda & 3) || (ldb & 3)) return AWARE_E_BADARG;
    launch_gemm_nt(A, lda, Bt, ldb, bias, C, ldc, M, N, K, (hipStream_t)stream);
    LAUNCHCHK();
    return AWARE_OK;
}
