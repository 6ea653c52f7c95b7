// Philox-4x32-10 and the Box-Muller pairing of the embed loop's attack chain (loop_attack_kernels.hip,
// loop_reverb_kernels.hip); the host twin is aware_amd/embedding/loop_attacks.py::philox4x32 / normal_draws.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace aware {

constexpr double kTwoToMinus32 = 2.3283064365386963e-10;

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned (&r)[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// whether an entry fires: (r0 + 0.5) / 2^32 < prob, in double as the host twin's fires()
__device__ __forceinline__ bool loop_entry_fires(unsigned r0, float prob) { return ((double)r0 + 0.5) * kTwoToMinus32 < (double)prob; }
// the draw of the entry a stage kernel serves, for clip b at the step the forward pass ran at:
// r = philox4x32_10((0, s, 1 + entry, 1), (seed_b, 0x5EED)); returns on
__device__ __forceinline__ bool loop_entry_draw(const LoopDraw& d, int b, unsigned (&r)[4]) {
    philox4x32_10(0u, (unsigned)(*d.step - d.step_back), 1u + (unsigned)d.entry, 1u, d.seeds[b], 0x5EEDu, r);
    return loop_entry_fires(r[0], d.prob);
}

// Box-Muller in f32 from the 32-bit lanes, arguments reduced in integers so that no bit of the draw is lost where it counts:
// radius sqrt(-2 ln u), u = (r + 0.5) / 2^32: the upper half of the range goes through log1p of the exact complement
__device__ __forceinline__ float bm_radius(unsigned r) {
    float w;
    if (r & 0x80000000u) w = -log1pf(-(((float)(0u - r) - 0.5f) * (float)kTwoToMinus32));
    else w = -logf(((float)r + 0.5f) * (float)kTwoToMinus32);
    return sqrtf(2.f * w);
}
// (cos, sin) of 2 pi (r + 0.5) / 2^32: the quadrant from the two top bits, the rest as a fraction of a quarter turn
__device__ __forceinline__ void bm_angle(unsigned r, float& c, float& s) {
    const float t = ((float)(r & 0x3FFFFFFFu) + 0.5f) * 9.313225746154785e-10f;      // / 2^30
    float sn, cs;
    sincospif(0.5f * t, &sn, &cs);
    const unsigned q = r >> 30;
    c = (q == 0) ? cs : (q == 1) ? -sn : (q == 2) ? -cs : sn;
    s = (q == 0) ? sn : (q == 1) ? cs : (q == 2) ? -sn : -cs;
}
// four standard normals of counter (blk, step, word, j): word 0 is the noise entries' stream, word 8 the impulse responses'
__device__ __forceinline__ void normal4w(unsigned blk, unsigned step, unsigned word, unsigned j, unsigned seed, float (&e)[4]) {
    unsigned r[4];
    philox4x32_10(blk, step, word, j, seed, 0x5EEDu, r);
    const float ra = bm_radius(r[0]), rb = bm_radius(r[2]);
    float c, s;
    bm_angle(r[1], c, s);
    e[0] = ra * c; e[1] = ra * s;
    bm_angle(r[3], c, s);
    e[2] = rb * c; e[3] = rb * s;
}
__device__ __forceinline__ void normal4(unsigned blk, unsigned step, unsigned j, unsigned seed, float (&e)[4]) {
    normal4w(blk, step, 0u, j, seed, e);
}

}  // namespace aware
