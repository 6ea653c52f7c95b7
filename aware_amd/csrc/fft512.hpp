// 1024-point real FFT / inverse real FFT for one 64-lane wavefront (gfx950).
//
// A frame is transformed by ONE wave: the 1024 real samples are packed into a
// 512-point complex sequence z[n] = x[2n] + i x[2n+1]; each lane keeps 8 complex
// values in registers and the transform is three radix-8 passes (512 = 8*8*8,
// decimation in frequency) with two transposes through a wave-private LDS
// scratch.  The real-FFT split / merge step pairs bin k with bin 512-k through
// the same scratch.  All cross-lane traffic happens at phase boundaries, so the
// phases are plain per-lane functions: on the device the 64 lanes run them in
// lock-step, and tests/host_sim runs them lane after lane on the CPU.
//
// Register <-> index convention everywhere ("natural order"):
//     lane L, register r  <->  element  L + 64*r     (L = 0..63, r = 0..7)
//
// Replaces torch.stft / torch.istft's per-frame rfft / irfft
// (reference: src/AWARE/utils/audio/stft.py:27-28, :47-48).
#pragma once
#include <hip/hip_runtime.h>

#define AW_HD __host__ __device__ __forceinline__

namespace aware {

constexpr int kNfft = 1024;       // frame length
constexpr int kHop = 256;         // hop
constexpr int kHalf = 512;        // complex FFT size
constexpr int kWave = 64;
// wave-private LDS scratch (cf units): the two exchanges below, and natural order
// 0..511 for the staged kernels' split / merge step.
constexpr int kFftScratch = 584;

// ---- where the two transposes sit in the scratch ----------------------------------
// Index functions of (lane, register), in cf units (8 bytes = 2 banks); the device
// phases and tests/host_sim/lds_bank_sim.cpp use this text.  The instruction on each
// side and its banking rule (lane groups that can conflict, bank of a 4-byte word):
//   stores  ds_write_b64 / ds_write2_b64   four groups of 16 consecutive lanes, word mod 32
//   loads   ds_read_b64 (lds_cf below)     two groups of 32 consecutive lanes,  word mod 64
// Exchange 1, element (k0, l = 8*n1 + n0) at k0*72 + l.  A store group writes 16
// consecutive cf.  A load group holds k0 = 4h..4h+3 and n0 = 0..7: 72*k0 is 8*k0 mod 32,
// so the 32 lanes read four runs of 8 cf that tile 32 cf = 64 banks.
AW_HD constexpr int xch1_store_index(int lane, int k0) { return k0 * 72 + lane; }
AW_HD constexpr int xch1_load_index(int lane, int n1) { return (lane >> 3) * 72 + 8 * n1 + (lane & 7); }
// Exchange 2, element (k0, q0, n0) at xch2_a(k0) + xch2_c(q0) + n0: separable, so both sides are
// one per-lane base plus a constant per register.  Each (k0, q0) owns a run of 8 cf (n0).  A store
// group holds two k0: a(2g+1) = a(2g) + 8, 16 consecutive cf.  A load group holds k0 = 0..7 and
// q0 = 4h..4h+3, whose 32 runs start at a + c = 33*j + 8*i + 264*h with j = (k0>>1) + 4*((q0>>1)&1)
// in 0..7 and i = (k0&1) + 2*(q0&1) in 0..3: every residue j + 8*i mod 32 once, so the 32 lanes of a
// load (equal n0) fall on 32 different cf of a 64-bank row.  The runs j + 8*i, i = 0..3, tile one row of
// 32 cf that starts at 33*j: the eight rows of a half h lie one cf apart, 264 cf per half, 528 in all.
// (The former k0*73 + 8*q0 + n0 loaded conflict-free but stored 2-way: k0 even, n0 = 0 and k0 odd,
// n0 = 7 met on one bank in every 16-lane group.  No linear pitch does both: the stores want the
// pitch = 8 mod 16, which puts k0 and k0 + 4 on the same banks for the loads.)
AW_HD constexpr int xch2_a(int k0) { return 33 * (k0 >> 1) + 8 * (k0 & 1); }
AW_HD constexpr int xch2_c(int q0) { return 132 * (q0 >> 1) + 16 * (q0 & 1); }
AW_HD constexpr int xch2_store_index(int lane, int q0) { return xch2_a(lane >> 3) + (lane & 7) + xch2_c(q0); }
AW_HD constexpr int xch2_load_index(int lane, int n0) { return xch2_a(lane & 7) + xch2_c(lane >> 3) + n0; }
// The step-2 twiddle table W64^(n0*q0) is symmetric, so it is read as [q0][n0]: the lanes of a
// load group read 8 consecutive cf (equal n0 broadcast).  Read as [n0][q0] (stride 8 cf = 16
// banks) n0 and n0 + 4 were two addresses on one bank for ds_read_b64, n0, n0 + 2, n0 + 4, n0 + 6
// four under the rule of ds_read2_b64 (16-lane groups, word mod 32).
AW_HD constexpr int tw2_index(int lane, int q0) { return q0 * 8 + (lane & 7); }

struct cf {
    float x, y;
};
AW_HD cf mk(float a, float b) { cf r; r.x = a; r.y = b; return r; }
AW_HD cf operator+(cf a, cf b) { return mk(a.x + b.x, a.y + b.y); }
AW_HD cf operator-(cf a, cf b) { return mk(a.x - b.x, a.y - b.y); }
AW_HD cf cmul(cf a, cf b) { return mk(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
AW_HD cf cconj(cf a) { return mk(a.x, -a.y); }
// One 8-byte LDS read as ONE ds_read_b64 (2 LDS cycles per wave, banks mod 64).  Left to itself the
// compiler pairs neighbouring reads into ds_read2_b64 / ds_read2st64_b64: 8 cycles for the two values
// instead of 4, banked mod 32 in 16-lane groups.  A volatile access is never paired; it is also never
// hoisted or dropped, which these reads (once per frame, by design) do not want either.  p is 8-byte
// aligned: the LDS arrays of cf are declared alignas(8).
// Per file: dsp_stream.hip defines AWARE_LDS_SINGLE_READS ahead of this header.  The workgroup-staged kernels of
// dsp_kernels.hip, off the hot path, keep plain loads and the pairing: that file is built with the SLP vectoriser, which
// packs their arithmetic according to the loads it finds, and their results would change in the last bit with it.
AW_HD cf lds_cf(const cf* p) {
#if defined(__HIP_DEVICE_COMPILE__) && defined(AWARE_LDS_SINGLE_READS)
    // The LDS address space is named: address-space inference leaves a volatile access on a generic pointer flat.
    // The value travels as one 64-bit integer, not as a float vector: a <2 x float> load makes the compiler keep the
    // arithmetic behind it packed (v_pk_fma_f32 ...), which contracts other products into FMAs than the scalar code does.
    const unsigned long long t = *(const volatile __attribute__((address_space(3))) unsigned long long*)p;
    return mk(__uint_as_float((unsigned)t), __uint_as_float((unsigned)(t >> 32)));
#else
    return *p;
#endif
}
// multiply by DIR*i  (DIR = -1: forward transform, +1: inverse)
template <int DIR> AW_HD cf mul_di(cf a) { return DIR > 0 ? mk(-a.y, a.x) : mk(a.y, -a.x); }

// In-register 8-point DFT: v[k] <- sum_n v[n] * exp(DIR * 2*pi*i * n*k / 8)
template <int DIR> AW_HD void radix8(cf (&v)[8]) {
    const float h = 0.70710678118654752440f;
    cf a0 = v[0] + v[4], a4 = v[0] - v[4];
    cf a1 = v[1] + v[5], a5 = v[1] - v[5];
    cf a2 = v[2] + v[6], a6 = v[2] - v[6];
    cf a3 = v[3] + v[7], a7 = v[3] - v[7];
    // twiddles w8^1, w8^2, w8^3 on the odd half
    cf t5 = mk(h * (a5.x - DIR * a5.y), h * (a5.y + DIR * a5.x));       // a5 * (1 + DIR i)/sqrt2
    cf t6 = mul_di<DIR>(a6);
    cf t7 = mk(h * (-a7.x - DIR * a7.y), h * (-a7.y + DIR * a7.x));     // a7 * (-1 + DIR i)/sqrt2
    // even outputs: DFT-4 of (a0,a1,a2,a3)
    cf c0 = a0 + a2, c2 = a0 - a2, c1 = a1 + a3, c3 = mul_di<DIR>(a1 - a3);
    v[0] = c0 + c1; v[4] = c0 - c1; v[2] = c2 + c3; v[6] = c2 - c3;
    // odd outputs: DFT-4 of (a4,t5,t6,t7)
    cf d0 = a4 + t6, d2 = a4 - t6, d1 = t5 + t7, d3 = mul_di<DIR>(t5 - t7);
    v[1] = d0 + d1; v[5] = d0 - d1; v[3] = d2 + d3; v[7] = d2 - d3;
}

// Per-lane twiddle constants, loaded once per wave from the plan's tables.
//   tw512[j]  = exp(-2*pi*i*j/512)   j = 0..511
//   tw1024[j] = exp(-2*pi*i*j/1024)  j = 0..511
struct FftLaneConst {
    cf t1[8];   // step-1 twiddle  W512^(lane*k0)
    cf t2[8];   // step-2 twiddle  W64^(n0*q0) = W512^(8*n0*q0)
};

AW_HD void fft_lane_const(int lane, const cf* tw512, FftLaneConst& c) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        c.t1[k] = tw512[(lane * k) & 511];
        c.t2[k] = tw512[(8 * (lane & 7) * k) & 511];
    }
}

template <int DIR> AW_HD cf tw_dir(cf w) { return DIR < 0 ? w : cconj(w); }

// ---- 512-point complex FFT in three lane-phases ---------------------------------
// phase A: radix-8 over r (stride 64), twiddle, scatter for transpose 1
template <int DIR> AW_HD void fft_phaseA(int lane, cf (&v)[8], const FftLaneConst& c, cf* s) {
    radix8<DIR>(v);
#pragma unroll
    for (int k0 = 0; k0 < 8; ++k0) {
        cf w = (k0 == 0) ? v[0] : cmul(v[k0], tw_dir<DIR>(c.t1[k0]));
        s[xch1_store_index(lane, k0)] = w;
    }
}
// phase B: gather (k0 = lane>>3, n0 = lane&7, reg = n1), radix-8, twiddle, scatter 2
template <int DIR> AW_HD void fft_phaseB(int lane, cf (&v)[8], const FftLaneConst& c, cf* s) {
#pragma unroll
    for (int n1 = 0; n1 < 8; ++n1) v[n1] = lds_cf(s + xch1_load_index(lane, n1));
    radix8<DIR>(v);
#pragma unroll
    for (int q0 = 0; q0 < 8; ++q0) {
        if (q0) v[q0] = cmul(v[q0], tw_dir<DIR>(c.t2[q0]));
    }
}
template <int DIR> AW_HD void fft_phaseB_store(int lane, const cf (&v)[8], cf* s) {
#pragma unroll
    for (int q0 = 0; q0 < 8; ++q0) s[xch2_store_index(lane, q0)] = v[q0];
}
// phase C: gather (k0 = lane&7, q0 = lane>>3, reg = n0), radix-8 -> natural order
template <int DIR> AW_HD void fft_phaseC(int lane, cf (&v)[8], cf* s) {
#pragma unroll
    for (int n0 = 0; n0 < 8; ++n0) v[n0] = lds_cf(s + xch2_load_index(lane, n0));
    radix8<DIR>(v);
}

// ---- the same phases with the twiddles read from LDS tables instead of registers ---------
// (28 VGPRs less per lane; tw1s[k0*64 + lane] = W512^(lane*k0): consecutive lanes read consecutive cf;
// tw2s[tw2_index(lane, q0)] = W64^(n0*q0); single ds_read_b64 each, conflict-free)
template <int DIR> AW_HD void fft_phaseA_t(int lane, cf (&v)[8], const cf* tw1s, cf* s) {
    radix8<DIR>(v);
#pragma unroll
    for (int k0 = 0; k0 < 8; ++k0) {
        cf w = (k0 == 0) ? v[0] : cmul(v[k0], tw_dir<DIR>(lds_cf(tw1s + k0 * 64 + lane)));
        s[xch1_store_index(lane, k0)] = w;
    }
}
template <int DIR> AW_HD void fft_phaseB_t(int lane, cf (&v)[8], const cf* tw2s, cf* s) {
#pragma unroll
    for (int n1 = 0; n1 < 8; ++n1) v[n1] = lds_cf(s + xch1_load_index(lane, n1));
    radix8<DIR>(v);
#pragma unroll
    for (int q0 = 1; q0 < 8; ++q0) v[q0] = cmul(v[q0], tw_dir<DIR>(lds_cf(tw2s + tw2_index(lane, q0))));
}
// fill the two tables (all threads of the block; caller synchronises)
AW_HD void fft_fill_tables(int tid, int nthreads, const cf* tw512, cf* tw1s, cf* tw2s) {
    for (int i = tid; i < 512; i += nthreads) tw1s[i] = tw512[((i & 63) * (i >> 6)) & 511];
    for (int i = tid; i < 64; i += nthreads) tw2s[i] = tw512[(8 * (i >> 3) * (i & 7)) & 511];
}

// ---- real-FFT split (forward) -----------------------------------------------------
// After the forward complex FFT, lane L reg r holds Z[L+64r].  X[k], k = 0..511:
//   X[k] = E - i*W^k*D,  E = (Z[k] + conj Z[512-k])/2,  D = (Z[k] - conj Z[512-k])/2
// phase 1: every lane stores its Z in natural order; phase 2: reads the partners.
AW_HD void rfft_split_store(int lane, const cf (&v)[8], cf* s) {
#pragma unroll
    for (int r = 0; r < 8; ++r) s[lane + 64 * r] = v[r];
}
// returns X[lane + 64*r]; tw1024 = exp(-2 pi i k/1024)
AW_HD cf rfft_split_bin(int k, cf zk, const cf* s, const cf* tw1024) {
    cf zp = s[(512 - k) & 511];
    cf e = mk(0.5f * (zk.x + zp.x), 0.5f * (zk.y - zp.y));
    cf d = mk(0.5f * (zk.x - zp.x), 0.5f * (zk.y + zp.y));
    cf w = tw1024[k];
    cf wd = cmul(w, d);
    return mk(e.x + wd.y, e.y - wd.x);      // e - i*wd
}
// X[512] = Re Z[0] - Im Z[0]  (purely real)
AW_HD float rfft_split_nyquist(const cf* s) { return s[0].x - s[0].y; }

// ---- inverse real FFT merge ---------------------------------------------------------
// Given the one-sided spectrum X[0..512], build Z[k] = E + i*O with
//   E = (X[k] + conj X[512-k])/2,  O = (X[k] - conj X[512-k])/2 * W^-k
// Then z = IFFT512(Z) (unnormalised) / 512 gives x[2n] = Re z[n], x[2n+1] = Im z[n]
// with irfft's 1/1024 normalisation folded in: scale = 1/512 * (the 1/2 above).
AW_HD cf irfft_merge_bin(int k, cf xk, cf xp /* X[512-k] */, const cf* tw1024) {
    cf e = mk(0.5f * (xk.x + xp.x), 0.5f * (xk.y - xp.y));
    cf d = mk(0.5f * (xk.x - xp.x), 0.5f * (xk.y + xp.y));
    cf w = cconj(tw1024[k]);           // W^-k
    cf o = cmul(d, w);
    return mk(e.x - o.y, e.y + o.x);   // e + i*o
}

#ifdef __HIPCC__
__device__ __forceinline__ void wave_sync() {
    // LDS ops of one wave execute in order; this only stops the compiler from
    // moving LDS accesses across the phase boundary.
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#endif
}
// Forward/inverse 512-point complex FFT of the wave's 8x64 values, natural order in
// and out.  `s` is this wave's private scratch (kFftScratch cf).
template <int DIR>
__device__ __forceinline__ void fft512_wave(int lane, cf (&v)[8], const FftLaneConst& c, cf* s) {
    fft_phaseA<DIR>(lane, v, c, s);
    wave_sync();
    fft_phaseB<DIR>(lane, v, c, s);
    wave_sync();
    fft_phaseB_store<DIR>(lane, v, s);
    wave_sync();
    fft_phaseC<DIR>(lane, v, s);
    wave_sync();
}
template <int DIR>
__device__ __forceinline__ void fft512_wave_t(int lane, cf (&v)[8], const cf* tw1s, const cf* tw2s, cf* s) {
    fft_phaseA_t<DIR>(lane, v, tw1s, s);
    wave_sync();
    fft_phaseB_t<DIR>(lane, v, tw2s, s);
    wave_sync();
    fft_phaseB_store<DIR>(lane, v, s);
    wave_sync();
    fft_phaseC<DIR>(lane, v, s);
    wave_sync();
}
#endif

}  // namespace aware
