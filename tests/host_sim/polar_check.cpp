// CPU check of polar_exact (aware_amd/csrc/polar.hpp): magnitude and unit phasor of a spectrum bin against hypot and atan2 in
// double, for components with exponents from -149 (the smallest subnormal) to +60, random mantissas and signs, the two
// components up to 40 binades apart, and bins with one or both components zero.
//
// The device takes the square root and the reciprocal from v_sqrt_f32 and v_rcp_f32, which read a subnormal operand as zero
// and return zero for a subnormal result.  FlushMath models exactly that on top of the host's correctly rounded sqrtf and
// division (the hardware's own error, 1 ulp each, is not modelled: the bars below leave room for it); multiplications and
// additions keep subnormals, as the kernels' do.  plain() is the form the kernels had, on the same model: it shows the bins
// that form loses, and polar_exact must return its bits wherever its sum of squares is at least 2^-100.
//
// Prints one line of `key value` pairs (tests/test_polar_host.py reads it).
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../aware_amd/csrc/polar.hpp"

namespace {

struct FlushMath {
    static float flush(float x) { return std::fabs(x) < FLT_MIN ? std::copysign(0.0f, x) : x; }
    static float sqrt(float x) { return flush(sqrtf(flush(x))); }
    static float rcp(float x) { return flush(1.0f / flush(x)); }
};

aware::Polar plain(float x, float y) {
    const float mg = FlushMath::sqrt(x * x + y * y);
    const float im = FlushMath::rcp(mg);
    return aware::Polar{mg, x * im, y * im};
}

uint32_t bits(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}
// a float with exponent e (subnormal below -126: rounded onto that grid) and a random mantissa and sign
float draw(int e) {
    const float m = 1.0f + (float)(rnd() & 0x7FFFFF) * 0x1p-23f;
    const float v = ldexpf(m, e);
    return (rnd() & 1) ? -v : v;
}
// the spacing of float32 at |v| (v in double)
double ulp_at(double v) {
    int e;
    std::frexp(std::fabs(v), &e);                  // |v| = f 2^e, f in [0.5, 1)
    return std::ldexp(1.0, (e - 1 < -126 ? -126 : e - 1) - 23);
}

struct Worst {
    double mag_ulp = 0, norm = 0, phase = 0;
    long n = 0, lost = 0, plain_lost = 0, differs = 0, compared = 0;
};

void one(float x, float y, Worst& w) {
    const aware::Polar p = aware::polar_exact<FlushMath>(x, y);
    const aware::Polar q = plain(x, y);
    const double ref = std::hypot((double)x, (double)y);
    ++w.n;
    if (q.mag == 0.f) ++w.plain_lost;
    if (!(p.mag > 0.f)) { ++w.lost; return; }
    w.mag_ulp = std::fmax(w.mag_ulp, std::fabs((double)p.mag - ref) / ulp_at(ref));
    w.norm = std::fmax(w.norm, std::fabs(std::hypot((double)p.ux, (double)p.uy) - 1.0));
    double d = std::atan2((double)p.uy, (double)p.ux) - std::atan2((double)y, (double)x);
    d = std::remainder(d, 2.0 * M_PI);
    w.phase = std::fmax(w.phase, std::fabs(d));
    if (x * x + y * y >= aware::kPolarFloor) {
        ++w.compared;
        if (bits(p.mag) != bits(q.mag) || bits(p.ux) != bits(q.ux) || bits(p.uy) != bits(q.uy)) ++w.differs;
    }
}

}  // namespace

int main() {
    static const int apart[] = {-40, -24, -12, -3, -1, 0, 1, 3, 12, 24, 40};
    Worst w;
    for (int e = -149; e <= 60; ++e) {
        for (int d : apart) {
            const int ey = e + d;
            if (ey < -149 || ey > 60) continue;
            for (int i = 0; i < 200; ++i) one(draw(e), draw(ey), w);
        }
        for (int i = 0; i < 50; ++i) { one(draw(e), 0.f, w); one(-0.f, draw(e), w); }
    }
    // the exact edges of the two forms: sums of squares on and next to 2^-100
    const float edge = 0x1p-50f;
    one(edge, 0.f, w); one(nextafterf(edge, 0.f), 0.f, w); one(nextafterf(edge, 1.f), 0.f, w);
    one(0.f, -edge, w); one(0x1p-51f, 0x1p-51f, w); one(0x1.6a09e6p-51f, 0x1.6a09e6p-51f, w);
    const aware::Polar z = aware::polar_exact<FlushMath>(0.f, 0.f), nz = aware::polar_exact<FlushMath>(-0.f, 0.f);
    std::printf("n %ld lost %ld plain_lost %ld mag_ulp %.4f norm %.3e phase %.3e compared %ld differs %ld zero_mag %d\n",
                w.n, w.lost, w.plain_lost, w.mag_ulp, w.norm, w.phase, w.compared, w.differs,
                (int)(bits(z.mag) == 0 && nz.mag == 0.f));
    return 0;
}
