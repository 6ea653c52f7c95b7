// The two scan kernel bodies (aware_amd/csrc/scan_body.hpp) on the CPU: no HIP header, no GPU.  Every thread of a workgroup is
// a fibre on one OS thread; threadIdx and blockIdx are shims, and the collective operations the bodies use (wave_sum, __ballot,
// __syncthreads) park the fibre until all threads of the workgroup have arrived, then hand every lane what the hardware would:
// the butterfly sum in common.hpp's order, the 64-bit vote of its wave.  Plain C++17 (build it with -ffp-contract=off, and
// with -fsanitize=address,undefined where wanted: the fibre switches are announced to AddressSanitizer).
//   scan_check in.bin out.bin
//   in:  int32 B, n_sync, L, max_flip, max_segments; float32 centre, min_confidence; int32 win_off[B + 1];
//        float32 values[W * n_sync * L]
//   out: win_conf[W] win_view[W] win_values[W * L] win_bits[W * words] n_seg[B] first last peak view conf [B * S] each,
//        values[B * S * L]; every segment array is filled with the int32 -7 before the run
#include <ucontext.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#if defined(__SANITIZE_ADDRESS__)
#define SCAN_ASAN 1
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
#define SCAN_ASAN 1
#endif
#endif
#ifdef SCAN_ASAN
#include <sanitizer/asan_interface.h>
#include <sanitizer/common_interface_defs.h>
#endif

// ---- the workgroup as fibres -------------------------------------------------------------------------------------------------------
namespace sim {

constexpr size_t kStack = 256 * 1024;

struct Index { int x = 0; };
Index thread_index, block_index;

struct Fibre {
    ucontext_t ctx;
    std::vector<char> stack;
    bool done = false;
    float f = 0.f;                  // what the thread brings to the collective, then what it takes away
    bool vote = false;
    unsigned long long mask = 0;
};

ucontext_t main_ctx;
const void* main_bottom = nullptr;
size_t main_size = 0;
std::vector<Fibre> fibres;
int current = -1;
std::function<void()> body;

void to_main(bool dying) {
    Fibre& f = fibres[current];
#ifdef SCAN_ASAN
    void* fake = nullptr;
    __sanitizer_start_switch_fiber(dying ? nullptr : &fake, main_bottom, main_size);
#endif
    swapcontext(&f.ctx, &main_ctx);
#ifdef SCAN_ASAN
    __sanitizer_finish_switch_fiber(fake, nullptr, nullptr);
#endif
    (void)dying;
}

void entry() {
#ifdef SCAN_ASAN
    __sanitizer_finish_switch_fiber(nullptr, &main_bottom, &main_size);
#endif
    body();
    fibres[current].done = true;
    to_main(true);
}

void resume(int i) {
    current = i;
    thread_index.x = i;
#ifdef SCAN_ASAN
    void* fake = nullptr;
    __sanitizer_start_switch_fiber(&fake, fibres[i].stack.data(), fibres[i].stack.size());
#endif
    swapcontext(&main_ctx, &fibres[i].ctx);
#ifdef SCAN_ASAN
    __sanitizer_finish_switch_fiber(fake, nullptr, nullptr);
#endif
}

// Park the calling thread until the whole workgroup is at a collective.
void rendezvous() {
    to_main(false);
    thread_index.x = current;
}

// One workgroup of `threads`: all fibres run to their next collective (or their end) in turn; the collectives' results are
// worked out per wave between the rounds.  The bodies reach every collective with all threads, in the same order.
void run_block(int block, int threads, const std::function<void()>& fn) {
    body = fn;
    block_index.x = block;
    fibres.resize(threads);
    for (Fibre& f : fibres) {
        f.stack.resize(kStack);
        f.done = false;
#ifdef SCAN_ASAN
        __asan_unpoison_memory_region(f.stack.data(), f.stack.size());     // what the fibre before left on it
#endif
        getcontext(&f.ctx);
        f.ctx.uc_stack.ss_sp = f.stack.data();
        f.ctx.uc_stack.ss_size = f.stack.size();
        f.ctx.uc_link = nullptr;
        makecontext(&f.ctx, entry, 0);
    }
    for (;;) {
        int alive = 0;
        for (int i = 0; i < threads; ++i)
            if (!fibres[i].done) {
                resume(i);
                alive += !fibres[i].done;
            }
        if (!alive) break;
        if (alive != threads) { fprintf(stderr, "threads left a collective behind\n"); exit(3); }
        for (int w0 = 0; w0 < threads; w0 += 64) {
            float s[64], n[64];
            unsigned long long mask = 0;
            for (int l = 0; l < 64; ++l) {
                s[l] = fibres[w0 + l].f;
                if (fibres[w0 + l].vote) mask |= 1ull << l;
            }
            for (int o = 32; o > 0; o >>= 1) {                 // common.hpp's wave_sum: v += __shfl_xor(v, o)
                for (int l = 0; l < 64; ++l) n[l] = s[l] + s[l ^ o];
                memcpy(s, n, sizeof s);
            }
            for (int l = 0; l < 64; ++l) { fibres[w0 + l].f = s[l]; fibres[w0 + l].mask = mask; }
        }
    }
}

}  // namespace sim

// ---- what the bodies name --------------------------------------------------------------------------------------------------------------
#define SCAN_HOST_SIM
#define SCAN_FN static inline
#define SCAN_SHARED static
#define threadIdx sim::thread_index
#define blockIdx sim::block_index

static float wave_sum(float v) {
    sim::Fibre& f = sim::fibres[sim::current];
    f.f = v; f.vote = false;
    sim::rendezvous();
    return sim::fibres[sim::current].f;
}
static unsigned long long __ballot(bool p) {
    sim::Fibre& f = sim::fibres[sim::current];
    f.f = 0.f; f.vote = p;
    sim::rendezvous();
    return sim::fibres[sim::current].mask;
}
static void __syncthreads() {
    sim::Fibre& f = sim::fibres[sim::current];
    f.f = 0.f; f.vote = false;
    sim::rendezvous();
}
static int __popc(unsigned v) { return __builtin_popcount(v); }
static int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static float __fadd_rn(float a, float b) { return a + b; }
static float __fsub_rn(float a, float b) { return a - b; }
static float __fmul_rn(float a, float b) { return a * b; }
static float __fdiv_rn(float a, float b) { return a / b; }

#include "../../aware_amd/csrc/scan_body.hpp"

template <class T>
static std::vector<T> read(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
template <class T>
static void write(FILE* f, const std::vector<T>& v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "short output\n"); exit(2); }
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: scan_check in.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    const std::vector<int32_t> head = read<int32_t>(in, 5);
    const int B = head[0], n = head[1], L = head[2], max_flip = head[3], S = head[4];
    const std::vector<float> par = read<float>(in, 2);
    if (B < 1 || n < 1 || n > 64 || L < 1 || L > aware::kScanMaxBits || max_flip < 0 || S < 1) { fprintf(stderr, "bad header\n"); return 2; }
    const std::vector<int32_t> off = read<int32_t>(in, (size_t)B + 1);
    for (int b = 0; b < B; ++b)
        if (off[0] != 0 || off[b + 1] < off[b]) { fprintf(stderr, "bad win_off\n"); return 2; }
    const int W = off[B], words = (L + 31) / 32;
    const std::vector<float> values = read<float>(in, (size_t)W * n * L);
    fclose(in);

    // exact sizes, so that AddressSanitizer sees any index outside them
    std::vector<float> win_conf(W), win_values((size_t)W * L);
    std::vector<int32_t> win_view(W);
    std::vector<uint32_t> win_bits((size_t)W * words);
    for (int w = 0; w < W; ++w)
        sim::run_block(w, 64, [&] {
            aware::scan_select_body(values.data(), n, L, par[0], win_conf.data(), win_view.data(), win_values.data(),
                                    win_bits.data());
        });

    const int32_t sentinel = -7;
    float fsentinel;
    memcpy(&fsentinel, &sentinel, 4);
    std::vector<int32_t> n_seg(B, sentinel), first((size_t)B * S, sentinel), last(first), peak(first), view(first);
    std::vector<float> conf((size_t)B * S, fsentinel), seg_values((size_t)B * S * L, fsentinel);
    for (int b = 0; b < B; ++b)
        sim::run_block(b, aware::kScanThreads, [&] {
            aware::scan_segments_body(win_conf.data(), win_view.data(), win_values.data(), win_bits.data(), off.data(), L, par[0],
                                      par[1], max_flip, S, n_seg.data(), first.data(), last.data(), peak.data(), view.data(),
                                      conf.data(), seg_values.data());
        });

    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    write(out, win_conf); write(out, win_view); write(out, win_values); write(out, win_bits); write(out, n_seg);
    write(out, first); write(out, last); write(out, peak); write(out, view); write(out, conf); write(out, seg_values);
    fclose(out);
    sim::fibres.clear();
    return 0;
}
