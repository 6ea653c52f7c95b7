// Magnitude and unit phasor of one spectrum bin, exact down to the smallest float32 (STFTDecomposer: torch.abs and
// torch.angle of a complex tensor, which go through hypot and atan2 and have no amplitude floor).
//
// The plain form  mg = sqrt(x x + y y), u = (x, y) / mg  loses a bin whose sum of squares leaves the normal range: the
// hardware square root and reciprocal (v_sqrt_f32, v_rcp_f32) read a subnormal operand as zero, so every bin with
// |X| < 2^-63 came out as magnitude 0 with the default phasor.  The waveform normaliser divides by max|x| + 1e-8, so a clip
// with peak p reaches the transform at about 1e8 p: clips with peaks below about 1e-27 lost every bin.
//
// polar_exact keeps the plain form, bit for bit, wherever the sum of squares is at least 2^-100, and below that takes the same
// three operations on the bin scaled by 2^100 (exact), scaling the magnitude back by 2^-100: components down to 2^-149
// then square to at least 2^-98.  Plain arithmetic, so the host compiles it too (tests/host_sim/polar_check.cpp); M supplies
// the square root and the reciprocal (HwMath in dsp_args.hpp on the device).
#pragma once
#ifndef AWARE_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define AWARE_HD __host__ __device__
#else
#define AWARE_HD
#endif
#endif

namespace aware {

constexpr float kPolarFloor = 0x1p-100f;     // sums of squares from here on take the plain form
constexpr float kPolarUp = 0x1p100f;
constexpr float kPolarDown = 0x1p-100f;

struct Polar {
    float mag;        // |X|
    float ux, uy;     // X / |X|; meaningless where mag == 0 (the caller stores its default there)
};

template <typename M>
AWARE_HD inline Polar polar_exact(float x, float y) {
    const float s = x * x + y * y;
    const bool tiny = !(s >= kPolarFloor);
    const float k = tiny ? kPolarUp : 1.0f;               // a product with 1 keeps the operand's bits
    const float xs = x * k, ys = y * k;
    const float ss = tiny ? xs * xs + ys * ys : s;
    const float mg = M::sqrt(ss);
    const float im = M::rcp(mg);
    Polar p;
    p.mag = tiny ? mg * kPolarDown : mg;
    p.ux = xs * im;
    p.uy = ys * im;
    return p;
}

}  // namespace aware
