// Real FFT / inverse real FFT of any power-of-two length N = 256 .. 4096 for one 64-lane wavefront (gfx950): the
// general-geometry STFT path (stft_any.hip).  The card's 1024-point transform keeps its own code (fft512.hpp).
//
// Same conventions as fft512.hpp:
//   - the N real samples are packed into the M = N/2 point complex sequence z[n] = x[2n] + i x[2n+1];
//   - the transform is a sequence of per-lane phase functions separated by wave_sync(), so tests/host_sim runs the
//     64 lanes one after another on the CPU;
//   - twiddles come from the plan's tables.
//
// The complex FFT is a Stockham auto-sort FFT in the wave's LDS scratch s[M] (natural order in and out).  Stage p
// (p = 1, r, r*r', ... the length of the sub-transforms already done) is a radix-r step:
//     u_m = s[j + m*M/r] * W_{p r}^{m k},   k = j mod p,   u <- DFT_r(u),   s[(j - k) r + k + m p] = u_m
// for the M/r butterflies j; lane L takes j = L + 64 i (i < M/(64 r)) and holds its M/64 inputs in registers
// between the load phase and the store phase of a stage.  Radix: 8 while it divides the rest, never more than M/64
// (so every lane has a butterfly): M = 128: 2^7, 256: 4^4, 512: 8^3, 1024: 8^3 2, 2048: 8^3 4.
#pragma once
#include "fft512.hpp"

namespace aware {
namespace fa {

// twiddle W_M^j = exp(-2 pi i j / M) from the half table th[j] = W_M^j, j < M/2 (W_M^{j + M/2} = -W_M^j)
template <int M> AW_HD cf tw_half(const cf* th, int j) {
    const cf w = th[j & (M / 2 - 1)];
    return (j & (M / 2)) ? mk(-w.x, -w.y) : w;
}

template <int DIR> AW_HD void radix2(cf* v) {
    const cf a = v[0], b = v[1];
    v[0] = a + b;
    v[1] = a - b;
}
template <int DIR> AW_HD void radix4(cf* v) {
    const cf a0 = v[0] + v[2], a1 = v[0] - v[2], a2 = v[1] + v[3], a3 = mul_di<DIR>(v[1] - v[3]);
    v[0] = a0 + a2;
    v[2] = a0 - a2;
    v[1] = a1 + a3;
    v[3] = a1 - a3;
}
template <int RAD, int DIR> AW_HD void radix(cf* v) {
    if constexpr (RAD == 2) radix2<DIR>(v);
    else if constexpr (RAD == 4) radix4<DIR>(v);
    else radix8<DIR>(*reinterpret_cast<cf(*)[8]>(v));
}

// radix of the stage that follows sub-transforms of length P
template <int M> constexpr int stage_radix(int P) {
    return (M / P < (M / 64 < 8 ? M / 64 : 8)) ? M / P : (M / 64 < 8 ? M / 64 : 8);
}

// ---- one Stockham stage as two lane phases --------------------------------------------------------------------
template <int M, int RAD> AW_HD void stage_load(int lane, cf* v, const cf* s) {
    constexpr int NB = M / (64 * RAD), T = M / RAD;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int m = 0; m < RAD; ++m) v[i * RAD + m] = s[lane + 64 * i + m * T];
}
template <int M, int P, int RAD, int DIR> AW_HD void stage_store(int lane, cf* v, cf* s, const cf* th) {
    constexpr int NB = M / (64 * RAD), STEP = M / (P * RAD);
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int j = lane + 64 * i, k = j & (P - 1);
        cf* u = v + i * RAD;
        if constexpr (P > 1) {
#pragma unroll
            for (int m = 1; m < RAD; ++m) u[m] = cmul(u[m], tw_dir<DIR>(tw_half<M>(th, m * k * STEP)));
        }
        radix<RAD, DIR>(u);
        const int base = (j - k) * RAD + k;
#pragma unroll
        for (int m = 0; m < RAD; ++m) s[base + m * P] = u[m];
    }
}

// ---- real-FFT split / inverse merge (the fft512.hpp formulas at size M; twN[k] = exp(-2 pi i k / 2M), k <= M) ----
// X[k], k = 0..M, from the forward complex FFT Z of the packed input (in s, natural order)
template <int M> AW_HD cf rfft_bin(int k, const cf* s, const cf* twN) {
    const cf zk = s[k & (M - 1)], zp = s[(M - k) & (M - 1)];
    const cf e = mk(0.5f * (zk.x + zp.x), 0.5f * (zk.y - zp.y));
    const cf d = mk(0.5f * (zk.x - zp.x), 0.5f * (zk.y + zp.y));
    const cf wd = cmul(twN[k], d);
    return mk(e.x + wd.y, e.y - wd.x);      // e - i*wd
}
// Z[k] = E + i*O of bin k from X[k] and X[M-k]; IFFT_M(Z) / M is then x[2n] + i x[2n+1] of irfft_N(X)
AW_HD cf irfft_merge(int k, cf xk, cf xp, const cf* twN) {
    const cf e = mk(0.5f * (xk.x + xp.x), 0.5f * (xk.y - xp.y));
    const cf d = mk(0.5f * (xk.x - xp.x), 0.5f * (xk.y + xp.y));
    const cf o = cmul(d, cconj(twN[k]));
    return mk(e.x - o.y, e.y + o.x);        // e + i*o
}
// lane phase of the merge: the row X[0..M] sits in s (s[M] = X[M]); lane L rewrites the pair (k, M-k), k = L + 64 i
// <= M/2, in place -- a pair's two reads and two writes belong to one lane
template <int M> AW_HD void irfft_merge_lane(int lane, cf* s, const cf* twN) {
#pragma unroll
    for (int i = 0; i <= M / 128; ++i) {
        const int k = lane + 64 * i;
        if (k > M / 2) break;
        const cf xk = s[k], xp = s[M - k];
        const cf zk = irfft_merge(k, xk, xp, twN);
        if (k != 0 && k != M / 2) s[M - k] = irfft_merge(M - k, xp, xk, twN);
        s[k] = zk;
    }
}

#ifdef __HIPCC__
template <int M, int P, int DIR> struct Stages {
    static constexpr int RAD = stage_radix<M>(P);
    __device__ __forceinline__ static void run(int lane, cf* v, cf* s, const cf* th) {
        stage_load<M, RAD>(lane, v, s);
        wave_sync();
        stage_store<M, P, RAD, DIR>(lane, v, s, th);
        wave_sync();
        if constexpr (P * RAD < M) Stages<M, P * RAD, DIR>::run(lane, v, s, th);
    }
};
// complex FFT (DIR -1) / unnormalised inverse (DIR +1) of s[0..M) in place; th: W_M half table (M/2 entries)
template <int M, int DIR> __device__ __forceinline__ void fft_wave(int lane, cf* s, const cf* th) {
    cf v[M / 64];
    Stages<M, 1, DIR>::run(lane, v, s, th);
}
#endif

}  // namespace fa
}  // namespace aware
