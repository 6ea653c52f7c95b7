// Sample deletion (EXTENSION, parity unpinned: the reference has Cropout and DeleteSamples as post-hoc attacks only and no
// chain inside its loop): k samples cut out of the clip at `start`, the remainder moved up, zeros at the end.  DESIGN.md
// section 21; the torch restatement is aware_amd/embedding/loop_attacks.py::delete_samples / apply_chain.
//
//   r = philox4x32_10((0, s, 1 + j, 1), (seed_b, 0x5EED)),  on = (r0 + 0.5) / 2^32 < prob,
//   k = k_lo + ((r2 * (k_hi - k_lo + 1)) >> 32)                          (k = 0 where the entry does not fire)
//   start = 0 (at: start) or (r1 * (Ny - k)) >> 32 (at: anywhere)
//   forward   z[i] = x[i] for i < start,  x[i + k] for start <= i < Ny - k,  0 for i >= Ny - k
//   adjoint   gx[i] = gz[i] for i < start,  0 for start <= i < start + k,  gz[i - k] for i >= start + k
//
// One kernel for both directions and both layouts.  Every value is a copy, so host and device agree bit for bit and k = 0 is
// the identity.  The source is misaligned by k against the destination, so every thread moves one float per step: a wave
// reads 256 consecutive bytes and writes 256 consecutive bytes, whatever k is.  Inside the loop one workgroup works through
// one synthesis run of a clip (the partition chain_kernel uses); the stand-alone entry runs on a grid over (chunk, clip) at
// any offset and length.
#include "common.hpp"
#include "kernels.h"
#include "loop_rng.hpp"

namespace aware {

namespace {

constexpr int kDsThreads = 256;
constexpr int kDsChunk = 8 * kDsThreads;        // samples per workgroup of the stand-alone grid

template <bool LOOP>
__global__ __launch_bounds__(kDsThreads) void delete_kernel(DeleteLaunch a) {
    const int b = blockIdx.y;
    const float* __restrict__ x;
    float* __restrict__ y;
    int n, i0, i1, start, k;        // the clip's length, this workgroup's samples [i0, i1), the cut [start, start + k)
    if (LOOP) {
        if (loop_gate_skips(a.draw.gate, b)) return;
        const int nblk = a.draw.frame_off[b + 1] - a.draw.frame_off[b] - 1;
        int nseg, jb0, jb1;
        synth_segment(nblk, blockIdx.x, a.draw.run_blocks, nseg, jb0, jb1);
        if ((int)blockIdx.x >= nseg) return;
        const int so = sig_offset(a.draw.frame_off, b);
        x = a.in + so; y = a.out + so;
        n = kHop * nblk;
        i0 = jb0 * kHop; i1 = jb1 * kHop;
        unsigned r[4];
        const bool on = loop_entry_draw(a.draw, b, r);
        k = on ? a.k_lo + (int)(((unsigned long long)r[2] * (unsigned long long)(unsigned)(a.k_hi - a.k_lo + 1)) >> 32) : 0;
        k = min(k, n);              // k_hi < Ny is checked where the chain is set
        start = (on && a.at) ? (int)(((unsigned long long)r[1] * (unsigned long long)(unsigned)(n - k)) >> 32) : 0;
    } else {
        n = a.len[b];
        x = a.in + a.off[b]; y = a.out + a.off[b];
        i0 = blockIdx.x * kDsChunk; i1 = min(i0 + kDsChunk, n);
        k = min(max(a.k[b], 0), max(n, 0));
        start = min(max(a.start[b], 0), n - k);
    }
    const int live = n - k;
    if (a.adjoint) {
        for (int i = i0 + threadIdx.x; i < i1; i += kDsThreads)
            y[i] = i < start ? x[i] : (i < start + k ? 0.f : x[i - k]);
    } else {
        for (int i = i0 + threadIdx.x; i < i1; i += kDsThreads)
            y[i] = i < start ? x[i] : (i < live ? x[i + k] : 0.f);
    }
}

}  // namespace

void launch_delete_samples(const DeleteLaunch& L, hipStream_t st) {
    if (L.draw.frame_off) {
        hipLaunchKernelGGL(delete_kernel<true>, dim3((unsigned)L.draw.pstride, (unsigned)L.B, 1), dim3(kDsThreads), 0, st, L);
    } else {
        const unsigned gx = (unsigned)((L.max_len + kDsChunk - 1) / kDsChunk);
        hipLaunchKernelGGL(delete_kernel<false>, dim3(gx, (unsigned)L.B, 1), dim3(kDsThreads), 0, st, L);
    }
}

}  // namespace aware
