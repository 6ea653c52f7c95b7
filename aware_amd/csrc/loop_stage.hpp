// What the stage kernels of the embed loop's splitting entries share (loop_speed_kernels.hip, loop_stretch_kernels.hip,
// loop_pitch_kernels.hip, loop_delete_kernels.hip, loop_filter_kernels.hip, loop_excerpt_kernels.hip, loop_warp_kernels.hip): the
// uniform integer draw, the workgroup's way into the loop's layout, the entry of the in -> out resamplers for both layouts, and
// the four-sample load and store.  Device helpers only.  DESIGN.md sections 17 to 21, 25, 32 and 35.
#pragma once
#include "common.hpp"
#include "kernels.h"
#include "loop_rng.hpp"

namespace aware {

// (r n) >> 32: uniform on [0, n) from one 32-bit lane, in integers as the host twin (loop_attacks.py) computes it
__device__ __forceinline__ int loop_below(unsigned r, int n) {
    return (int)(((unsigned long long)r * (unsigned long long)(unsigned)n) >> 32);
}
// lo + ((r (hi - lo + 1)) >> 32): uniform on [lo, hi]
__device__ __forceinline__ int loop_uniform(unsigned r, int lo, int hi) { return lo + loop_below(r, hi - lo + 1); }

// one workgroup's share of clip b in the embed loop's layout, and the draw of the entry the kernel serves
struct LoopStage {
    int so, n;          // the clip: n = Ny_b floats at offset so of every signal array
    int jb0, jb1;       // this workgroup's hop blocks [jb0, jb1): one synthesis run, the partition chain_kernel uses
    bool on;            // whether the entry fires on this clip at this step
    unsigned r[4];      // its draw
};
// False where the workgroup has nothing to do: a clip that drew another chain of a mixture, or a run the clip does not have.
// Every condition depends on blockIdx and per-clip data only, so `if (!loop_stage_enter(...)) return;` is uniform across the
// workgroup: the pitch and filter kernels place __syncthreads() after it.  Keep it that way.  A kernel calls it directly, not
// through a second helper that hands the result on: the early returns then compile to the branches they are.
__device__ __forceinline__ bool loop_stage_enter(const LoopDraw& d, int b, LoopStage& s) {
    if (loop_gate_skips(d.gate, b)) return false;
    const int nblk = d.frame_off[b + 1] - d.frame_off[b] - 1;
    int nseg;
    synth_segment(nblk, blockIdx.x, d.run_blocks, nseg, s.jb0, s.jb1);
    if ((int)blockIdx.x >= nseg) return false;
    s.so = sig_offset(d.frame_off, b);
    s.n = kHop * nblk;
    s.on = loop_entry_draw(d, b, s.r);
    return true;
}

// The way into a resampler (ResampleLaunch) for both layouts; in the loop `s` is what loop_stage_enter gave.  x and y, the
// lengths of the x side and the z side, this workgroup's groups of four outputs [q0, q1) and the offset m (0 where the entry
// does not fire, and behind a phase vocoder that drew its stretch mode: `coin`, DESIGN.md section 20, which only a kernel with
// COIN reads: the speed change)
template <bool LOOP, bool COIN = false>
__device__ __forceinline__ void resample_enter(const ResampleLaunch& a, int b, const LoopStage& s, const float*& x, float*& y,
                                               int& nx, int& nz, int& q0, int& q1, int& m) {
    if (LOOP) {
        x = a.in + s.so; y = a.out + s.so;
        nx = nz = s.n;
        q0 = s.jb0 * (kHop / 4); q1 = s.jb1 * (kHop / 4);
        m = s.on ? loop_uniform(s.r[3], a.m_lo, a.m_hi) : 0;
        if (COIN && a.coin && s.r[2] < 0x80000000u) m = 0;
    } else {
        nx = a.x_len[b]; nz = a.z_len[b];
        x = a.in + (a.adjoint ? a.z_off[b] : a.x_off[b]);
        y = a.out + (a.adjoint ? a.x_off[b] : a.z_off[b]);
        q0 = blockIdx.x * kResampleThreads; q1 = q0 + kResampleThreads;
        m = a.m[b];
    }
}

// v = x[i .. i + 3], zero from n on: the identity of m = 0, exactly
__device__ __forceinline__ void load4(const float* x, int n, int i, float v[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = i + e < n ? x[i + e] : 0.f;
}
// y[4 q .. 4 q + 3] = v: one float4 in the loop, which the 256-float clip alignment allows; stand-alone at any offset, scalars
// below n
template <bool LOOP>
__device__ __forceinline__ void store4(float* y, int n, int q, const float v[4]) {
    if (LOOP) {
        reinterpret_cast<float4*>(y)[q] = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * q + e < n) y[4 * q + e] = v[e];
    }
}

}  // namespace aware
