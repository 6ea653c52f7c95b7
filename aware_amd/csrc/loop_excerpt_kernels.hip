// Tiled excerpt (EXTENSION, parity unpinned: the reference has Cropout as a post-hoc attack only and no chain inside its loop):
// what a detector sees of the excerpt [start, start + L) of the clip.  The excerpt is repeated periodically until it fills the
// clip, so the clip keeps its length, and the detector's norms and its read-out's mean see the excerpt's own statistics.
// DESIGN.md section 32; the torch restatement is aware_amd/embedding/loop_attacks.py::excerpt_tile / apply_chain.
//
//   r = philox4x32_10((0, s, 1 + j, 1), (seed_b, 0x5EED)),  on = (r0 + 0.5) / 2^32 < prob,
//   L = min(L_lo + ((r2 * (L_hi - L_lo + 1)) >> 32), Ny)                  (L = Ny where the entry does not fire)
//   start = (r1 * (Ny - L + 1)) >> 32
//   forward   z[i] = x[start + (i mod L)]
//   adjoint   gx[i] = sum_m gz[(i - start) + m L] for start <= i < start + L, m = 0, 1, .. while the index is below Ny; +0.0 outside
//
// One kernel for both directions and both layouts.  The forward pass copies, and the adjoint adds in f32 with m ascending: the
// accumulator starts as the first term and takes one __fadd_rn per further term, which is what the host twin does, so the two
// agree bit for bit and L = Ny is the identity.  No division per sample: a thread takes i mod L once and walks on with a
// conditional subtract (the stride of 256 is below kExcerptMinLen; the stand-alone entry, which accepts any L >= 1, reduces
// the stride modulo L once).  Forward, a wave reads 256 consecutive bytes but for one wrap per period; adjoint, it reads 256
// consecutive bytes per term.  Inside the loop one workgroup works through one synthesis run of a clip (the partition
// chain_kernel uses); the stand-alone entry runs on a grid over (chunk, clip) at any offset and length.
#include "loop_stage.hpp"

namespace aware {

namespace {

constexpr int kExThreads = 256;
constexpr int kExChunk = 8 * kExThreads;        // samples per workgroup of the stand-alone grid

template <bool LOOP>
__global__ __launch_bounds__(kExThreads) void excerpt_kernel(ExcerptLaunch a) {
    const int b = blockIdx.y;
    const float* __restrict__ x;
    float* __restrict__ y;
    int n, i0, i1, start, len;      // the clip's length, this workgroup's samples [i0, i1), the excerpt [start, start + len)
    if (LOOP) {
        LoopStage s;
        if (!loop_stage_enter(a.draw, b, s)) return;
        x = a.in + s.so; y = a.out + s.so;
        n = s.n;
        i0 = s.jb0 * kHop; i1 = s.jb1 * kHop;
        len = s.on ? min(loop_uniform(s.r[2], a.l_lo, a.l_hi), n) : n;
        start = loop_below(s.r[1], n - len + 1);
    } else {
        n = a.len[b];
        if (n < 1) return;
        x = a.in + a.off[b]; y = a.out + a.off[b];
        i0 = blockIdx.x * kExChunk; i1 = min(i0 + kExChunk, n);
        len = min(max(a.length[b], 1), n);
        start = min(max(a.start[b], 0), n - len);
    }
    const unsigned un = (unsigned)n, ul = (unsigned)len;      // p + len stays below 2 n, inside 32 bits
    if (a.adjoint) {
        for (int i = i0 + threadIdx.x; i < i1; i += kExThreads) {
            float acc = 0.f;
            if (i >= start && i - start < len) {
                unsigned q = (unsigned)(i - start);
                acc = x[q];
                for (q += ul; q < un; q += ul) acc = __fadd_rn(acc, x[q]);
            }
            y[i] = acc;
        }
    } else {
        const unsigned step = len > kExThreads ? (unsigned)kExThreads : (unsigned)kExThreads % ul;
        unsigned p = (unsigned)(i0 + (int)threadIdx.x) % ul;
        for (int i = i0 + threadIdx.x; i < i1; i += kExThreads) {
            y[i] = x[(unsigned)start + p];
            p += step;
            if (p >= ul) p -= ul;
        }
    }
}

}  // namespace

void launch_excerpt_tile(const ExcerptLaunch& L, hipStream_t st) {
    hipLaunchKernelGGL(L.draw.frame_off ? excerpt_kernel<true> : excerpt_kernel<false>, stage_grid(L.draw, L.B, L.max_len, kExChunk),
                       dim3(kExThreads), 0, st, L);
}

}  // namespace aware
