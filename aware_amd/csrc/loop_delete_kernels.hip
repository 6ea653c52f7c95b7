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
#include "loop_stage.hpp"

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
        LoopStage s;
        if (!loop_stage_enter(a.draw, b, s)) return;
        x = a.in + s.so; y = a.out + s.so;
        n = s.n;
        i0 = s.jb0 * kHop; i1 = s.jb1 * kHop;
        k = s.on ? loop_uniform(s.r[2], a.k_lo, a.k_hi) : 0;
        k = min(k, n);              // k_hi < Ny is checked where the chain is set
        start = (s.on && a.at) ? loop_below(s.r[1], n - k) : 0;
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
    hipLaunchKernelGGL(L.draw.frame_off ? delete_kernel<true> : delete_kernel<false>, stage_grid(L.draw, L.B, L.max_len, kDsChunk),
                       dim3(kDsThreads), 0, st, L);
}

}  // namespace aware
