// The Viterbi kernel body (aware_amd/csrc/viterbi_body.hpp) on the CPU: no HIP header, no GPU.  The body is written in wave
// statements (see its head); here a VitWave<T> is 64 values, VIT_LANES a loop over the 64 lanes, and the operations that cross
// the lanes are plain indexing: the cross-lane read takes lane src's value, the ballot gathers the 64 votes.  The rounding
// intrinsics are the C operators.  Plain C++17 (build it with -ffp-contract=off, and with -fsanitize=address,undefined where
// wanted); every buffer has its exact size, so that AddressSanitizer sees any index outside it.
//   viterbi_check in.bin out.bin
//   in:  int32 R, L, n, c; float32 centre; float32 values[R * L]
//   out: uint32 bits[R * ceil(L / n / 32)]; float32 metric[R]; int32 valid[R]; int32 corrected[R]; every array is filled with
//        the int32 -7 before the run
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// ---- what the body names ---------------------------------------------------------------------------------------------------------
#define VITERBI_HOST_SIM
#define VIT_FN static inline
template <class T> struct VitWave { T v[64]; };
#define VIT_LANES(d) for (int d = 0; d < 64; ++d)
#define VIT_AT(x, d) ((x).v[d])
#define VIT_READ(x, src) ((x).v[src])
#define VIT_READ_U(x, src) ((x).v[src])
#define VIT_BALLOT(x) vit_ballot(x)

static unsigned long long vit_ballot(const VitWave<bool>& p) {
    unsigned long long m = 0;
    for (int l = 0; l < 64; ++l)
        if (p.v[l]) m |= 1ull << l;
    return m;
}
static int __popc(unsigned v) { return __builtin_popcount(v); }
static float __fadd_rn(float a, float b) { return a + b; }
static float __fsub_rn(float a, float b) { return a - b; }
static unsigned __float_as_uint(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static float __uint_as_float(unsigned u) { float f; memcpy(&f, &u, 4); return f; }

#include "../../aware_amd/csrc/viterbi_body.hpp"

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
    if (argc != 3) { fprintf(stderr, "usage: viterbi_check in.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    const std::vector<int32_t> head = read<int32_t>(in, 4);
    const int R = head[0], L = head[1], n = head[2], c = head[3];
    const float centre = read<float>(in, 1)[0];
    // what aware_viterbi_decode checks before it launches
    if (R < 1 || R > (1 << 20) || L < 1 || L > aware::kViterbiMaxBits || (n != 2 && n != 3) || (c != 0 && c != 8 && c != 16) ||
        !std::isfinite(centre) || L / n - 6 - c < 1) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    const std::vector<float> values = read<float>(in, (size_t)R * L);
    fclose(in);

    const int words = (L / n + 31) / 32;
    const int32_t sentinel = -7;
    float fsentinel;
    memcpy(&fsentinel, &sentinel, 4);
    std::vector<uint32_t> bits((size_t)R * words, (uint32_t)sentinel);
    std::vector<float> metric(R, fsentinel);
    std::vector<int32_t> valid(R, sentinel), corrected(R, sentinel);
    const int groups = (R + aware::kViterbiRows - 1) / aware::kViterbiRows;        // the launch's grid and its four waves
    for (int group = 0; group < groups; ++group)
        for (int wave = 0; wave < aware::kViterbiRows; ++wave)
            aware::viterbi_body(values.data(), R, L, centre, n, c, group, wave, bits.data(), metric.data(), valid.data(),
                                corrected.data());

    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    write(out, bits); write(out, metric); write(out, valid); write(out, corrected);
    fclose(out);
    return 0;
}
