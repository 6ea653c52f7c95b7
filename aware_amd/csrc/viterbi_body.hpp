// The body of the Viterbi kernel (viterbi_kernels.hip), apart from the launch indices, so that
// tests/host_sim/viterbi_check.cpp can compile the same text for the host.  DESIGN.md section 29; the restatement is
// aware_amd/utils/watermark/fec.py (viterbi_decode).
//
// One wave decodes one row; lane d is trellis state d.  The text is written in wave statements: a VitWave<T> is one value per
// lane, VIT_LANES(d) { ... } is what every lane d does, and three operations cross the lanes: VIT_READ (any lane's value, the
// index per lane), VIT_READ_U (one lane's value for the whole wave, the index uniform) and VIT_BALLOT.  On the device a
// VitWave<T> is a register, VIT_LANES runs its block once with d the lane index, and the three are __shfl, v_readlane and
// __ballot.  The host check defines VITERBI_HOST_SIM and supplies: VitWave<T> as 64 values, VIT_LANES as a loop over them, the
// three as plain indexing, and __fadd_rn, __fsub_rn, __popc, __float_as_uint.  One rule makes both readings agree: a
// VIT_LANES block never reads through VIT_READ a value that the same block writes (the new metrics go to `nm`, and a
// second block copies them).
#pragma once

#ifndef VITERBI_HOST_SIM
#define VIT_FN __device__ __forceinline__
template <class T> using VitWave = T;
#define VIT_LANES(d) for (int d = (int)(threadIdx.x & 63), once_ = 1; once_; once_ = 0)
#define VIT_AT(x, d) (x)
#define VIT_READ(x, src) __shfl((x), (src))
#define VIT_READ_U(x, src) aware::vit_readlane((x), (src))
#define VIT_BALLOT(x) __ballot(x)
#endif

namespace aware {

#ifdef VITERBI_HOST_SIM
constexpr int kViterbiMaxBits = 512;                   // as kernels.h has them
constexpr int kViterbiRows = 4;
#else
VIT_FN unsigned vit_readlane(unsigned v, int lane) { return (unsigned)__builtin_amdgcn_readlane((int)v, lane); }
VIT_FN float vit_readlane(float v, int lane) { return __uint_as_float(vit_readlane(__float_as_uint(v), lane)); }
VIT_FN unsigned long long vit_readlane(unsigned long long v, int lane) {
    return ((unsigned long long)vit_readlane((unsigned)(v >> 32), lane) << 32) | vit_readlane((unsigned)v, lane);
}
#endif

constexpr int kViterbiTail = 6;
constexpr int kViterbiChunk = 64;                      // steps whose survivor words one register per lane holds
constexpr int kViterbiChunks = kViterbiMaxBits / 2 / kViterbiChunk;     // T <= 256: four registers

// generator g of the code with n outputs per step
VIT_FN unsigned vit_poly(int n, int g) { return n == 2 ? (g == 0 ? 0171u : 0133u) : (g == 0 ? 0133u : g == 1 ? 0171u : 0165u); }
VIT_FN unsigned vit_parity(unsigned v) { return (unsigned)__popc(v) & 1u; }
VIT_FN bool vit_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
// y = v - centre, 0 where that is not finite (an erasure)
VIT_FN float vit_soft(float v, float centre) {
    const float y = __fsub_rn(v, centre);
    return vit_finite(y) ? y : 0.f;
}
VIT_FN float vit_signed(float y, unsigned flip) { return __uint_as_float(__float_as_uint(y) ^ flip); }

// The sign-bit masks of a lane's two incoming branches: flip[3 x + g] negates y_g on the branch from predecessor s_x.
struct VitSigns { VitWave<unsigned> flip[6]; };

// The soft values of the steps t0 .. t1 - 1 (at most 64 of them, t0 a multiple of 64), read once: lane t % 64 holds
// y_nt+g in g[g], and a step takes its values from there with VIT_READ_U instead of waiting for memory.
struct VitSoft { VitWave<float> g[3]; };
VIT_FN void vit_load(const float* __restrict__ v, int t0, int t1, int n, float centre, VitSoft& y) {
    VIT_LANES(d) {
        for (int g = 0; g < 3; ++g) VIT_AT(y.g[g], d) = g < n && t0 + d < t1 ? vit_soft(v[n * (t0 + d) + g], centre) : 0.f;
    }
}

// Steps t0 .. t1 - 1: lane t % 64 keeps step t's survivor word in sv.
VIT_FN void vit_forward(const float* __restrict__ v, int t0, int t1, int n, float centre, const VitSigns& sg,
                        VitWave<float>& pm, VitWave<unsigned long long>& sv) {
    VitWave<float> nm;
    VitWave<bool> take;
    VitSoft y;
    vit_load(v, t0, t1, n, centre, y);
    for (int t = t0; t < t1; ++t) {
        const float y0 = VIT_READ_U(y.g[0], t & 63), y1 = VIT_READ_U(y.g[1], t & 63);
        const float y2 = n == 3 ? VIT_READ_U(y.g[2], t & 63) : 0.f;
        VIT_LANES(d) {
            float m0 = VIT_READ(pm, 2 * (d & 31)), m1 = VIT_READ(pm, 2 * (d & 31) + 1);
            m0 = __fadd_rn(__fadd_rn(m0, vit_signed(y0, VIT_AT(sg.flip[0], d))), vit_signed(y1, VIT_AT(sg.flip[1], d)));
            m1 = __fadd_rn(__fadd_rn(m1, vit_signed(y0, VIT_AT(sg.flip[3], d))), vit_signed(y1, VIT_AT(sg.flip[4], d)));
            if (n == 3) {
                m0 = __fadd_rn(m0, vit_signed(y2, VIT_AT(sg.flip[2], d)));
                m1 = __fadd_rn(m1, vit_signed(y2, VIT_AT(sg.flip[5], d)));
            }
            const bool x = m1 > m0;                    // a tie, or a NaN, goes to x = 0
            VIT_AT(take, d) = x;
            VIT_AT(nm, d) = x ? m1 : m0;
        }
        const unsigned long long word = VIT_BALLOT(take);
        VIT_LANES(d) {
            VIT_AT(pm, d) = VIT_AT(nm, d);
            if (d == (t & 63)) VIT_AT(sv, d) = word;
        }
    }
}

// The same steps backwards on the wave-uniform path: from state s after step t1 - 1 to the state before step t0.  Step t's
// input bit goes to bit t % 32 of lane t / 32's word, and the branch's output bits are held against the signs of y.
VIT_FN void vit_traceback(const float* __restrict__ v, int t0, int t1, int n, float centre,
                          const VitWave<unsigned long long>& sv, int& s, int& corrected, VitWave<unsigned>& out) {
    VitSoft y;
    vit_load(v, t0, t1, n, centre, y);
    for (int t = t1 - 1; t >= t0; --t) {
        const unsigned long long word = VIT_READ_U(sv, t & 63);
        const int b = s >> 5, prev = ((s & 31) << 1) | (int)((word >> s) & 1ull);
        const unsigned r = (unsigned)((b << 6) | prev);
        for (int g = 0; g < 3; ++g)
            if (g < n) corrected += (int)((VIT_READ_U(y.g[g], t & 63) > 0.f) != (vit_parity(r & vit_poly(n, g)) != 0u));
        VIT_LANES(d) {
            if (d == (t >> 5)) VIT_AT(out, d) |= (unsigned)b << (t & 31);
        }
        s = prev;
    }
}

// Wave `wave` of workgroup `group` decodes row group * kViterbiRows + wave of values [R][L]: bits [R][ceil(T / 32)],
// metric, valid, corrected [R].  n in {2, 3}, c in {0, 8, 16}, T = L / n in 7 + c .. 256 (the entry checks them).
VIT_FN void viterbi_body(const float* __restrict__ values, int R, int L, float centre, int n, int c, int group, int wave,
                         unsigned* __restrict__ bits, float* __restrict__ metric, int* __restrict__ valid,
                         int* __restrict__ corrected) {
    const int row = group * kViterbiRows + wave;
    if (row >= R) return;                              // the whole wave leaves
    const int T = L / n, k = T - kViterbiTail - c, words = (T + 31) / 32;
    const float* v = values + (size_t)row * L;

    VitSigns sg;
    VitWave<float> pm;
    VitWave<unsigned> out;
    VitWave<unsigned long long> sv0, sv1, sv2, sv3;
    VIT_LANES(d) {
        for (int x = 0; x < 2; ++x) {
            const unsigned r = (unsigned)(((d >> 5) << 6) | ((d & 31) << 1) | x);
            for (int g = 0; g < 3; ++g) VIT_AT(sg.flip[3 * x + g], d) = g < n && vit_parity(r & vit_poly(n, g)) ? 0u : 0x80000000u;
        }
        VIT_AT(pm, d) = d == 0 ? 0.f : __uint_as_float(0xff800000u);       // -inf
        VIT_AT(out, d) = 0u;
        VIT_AT(sv0, d) = 0ull; VIT_AT(sv1, d) = 0ull; VIT_AT(sv2, d) = 0ull; VIT_AT(sv3, d) = 0ull;
    }
    static_assert(kViterbiChunks == 4, "four survivor registers per lane");
    const int e0 = T < 64 ? T : 64, e1 = T < 128 ? T : 128, e2 = T < 192 ? T : 192;
    vit_forward(v, 0, e0, n, centre, sg, pm, sv0);
    if (T > 64) vit_forward(v, 64, e1, n, centre, sg, pm, sv1);
    if (T > 128) vit_forward(v, 128, e2, n, centre, sg, pm, sv2);
    if (T > 192) vit_forward(v, 192, T, n, centre, sg, pm, sv3);
    const float final_metric = VIT_READ_U(pm, 0);

    int s = 0, wrong = 0;
    if (T > 192) vit_traceback(v, 192, T, n, centre, sv3, s, wrong, out);
    if (T > 128) vit_traceback(v, 128, e2, n, centre, sv2, s, wrong, out);
    if (T > 64) vit_traceback(v, 64, e1, n, centre, sv1, s, wrong, out);
    vit_traceback(v, 0, e0, n, centre, sv0, s, wrong, out);

    // the CRC of the k message bits, serially on the uniform path, against the c bits that follow them
    bool ok = vit_finite(final_metric);
    if (c > 0) {
        const unsigned poly = c == 8 ? 0x07u : 0x1021u, mask = (1u << c) - 1u;
        unsigned reg = mask, got = 0u;
        for (int t = 0; t < k + c; ++t) {
            const unsigned b = (VIT_READ_U(out, t >> 5) >> (t & 31)) & 1u;
            if (t < k) reg = ((reg << 1) & mask) ^ ((((reg >> (c - 1)) ^ b) & 1u) ? poly : 0u);
            else got = (got << 1) | b;
        }
        ok = ok && got == reg;
    }
    VIT_LANES(d) {
        if (d < words) bits[(size_t)row * words + d] = VIT_AT(out, d);
        if (d == 0) { metric[row] = final_metric; valid[row] = ok ? 1 : 0; corrected[row] = wrong; }
    }
}

}  // namespace aware
