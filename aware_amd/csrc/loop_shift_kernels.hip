// Frequency shift (EXTENSION, parity unpinned: the reference has no single-sideband attack and no chain inside its loop): every
// component of the clip moved by the same number of Hz, through a 255-tap Hilbert transformer and a phase that is exact in
// integers.  DESIGN.md section 37; the torch restatement is aware_amd/embedding/loop_attacks.py::hilbert_taps / frequency_shift.
//
//   r = philox4x32_10((0, s, 1 + j, 1), (seed_b, 0x5EED)),  on = (r0 + 0.5) / 2^32 < prob,
//   d = d_lo + ((r1 * (d_hi - d_lo + 1)) >> 32): the shift in units of sr / 2^20 Hz, signed, |d| <= 65536;  p0 = r2 >> 12
//   w[k] = 0.54 + 0.46 cos(pi k / 127),  h[k] = w[k] 2 / (pi k) for odd k, 0 for even k, k = -127..127: h[-k] = -h[k]
//   (Hx)[i] = sum_k h[k] x[i - k], x zero outside the clip
//   theta_i = (p0 + i d) mod 2^20 (a wrapping 32-bit multiply-add and & 0xFFFFF),  phi_i = 2 pi theta_i / 2^20
//   forward  z[i]  = x[i] cos phi_i - (Hx)[i] sin phi_i                a positive d shifts upwards
//   adjoint  gx[j] = g[j] cos phi_j + (H(g sin phi))[j]                exact: H^T = -H under the extension by zeros
//
// One kernel for both layouts and both directions; the adjoint multiplies by sin phi while staging and adds g cos phi at the
// store.  Half the taps are zero: an even output reads odd inputs only and an odd output even inputs only, and with the tile
// staged from an even sample on, both are the same 128-tap filter g[u] = h[127 - 2 u] on the other parity's plane:
//   Hx[2 a] = sum_u g[u] P1[a + u],  Hx[2 a + 1] = sum_u g[u] P0[a + 1 + u],  P0[m] = staged[2 m], P1[m] = staged[2 m + 1].
// A workgroup serves up to kFsTile consecutive outputs at a time: it stages them with 128 samples in front and the halo behind
// into the two planes (zeros outside the clip, whatever lies beside it in memory), builds the 64 distinct tap magnitudes, and
// every thread produces the 8 even and the 8 odd outputs of 16 consecutive samples.  The pair shares its taps, so each tap is one
// packed FMA on both: 128 FMAs per output.  The two windows of 8 samples slide through registers.  LDS: plane index p lives at
// p + (p >> 3), so thread t, which reads 8 t + const, has stride 9 and a wave's 32-lane groups touch 32 banks (unpadded: 8);
// the plane of the even samples starts 16 banks (mod 32) from the other, so the staging store of 32 consecutive samples, 16 to
// each plane, touches a bank twice at most, which a 4-byte store absorbs.  The taps are read at one address by the whole wave.  The tile body (staging, taps, accumulation)
// is shift_hilbert.hpp, which the shift search's kernel (shift_search_kernels.hip) includes as well.
#include "loop_stage.hpp"
#include "shift_hilbert.hpp"

namespace aware {

namespace {

template <bool LOOP, bool ADJOINT>
__global__ __launch_bounds__(kFsThreads) void frequency_shift_kernel(ShiftLaunch a) {
    __shared__ float xs[2 * kFsPlanePhys];      // P1 (odd staged samples), then P0
    __shared__ __attribute__((aligned(16))) float hs[kFsTaps];       // g[u] = h[127 - 2 u]
    const int b = blockIdx.y;
    const int t = threadIdx.x;
    const float* __restrict__ x;
    float* __restrict__ y;
    int n, i0, i1, d, p0;                       // the clip's length, this workgroup's outputs [i0, i1), the shift and the start phase
    bool on = true;
    if (LOOP) {
        LoopStage s;
        if (!loop_stage_enter(a.draw, b, s)) return;
        x = a.in + s.so; y = a.out + s.so;
        n = s.n;
        i0 = s.jb0 * kHop; i1 = s.jb1 * kHop;
        d = loop_uniform(s.r[1], a.d_lo, a.d_hi);
        p0 = (int)(s.r[2] >> 12);
        on = s.on;
    } else {
        n = a.len[b];
        i0 = blockIdx.x * kFsTile;
        if (i0 >= n) return;
        i1 = min(i0 + kFsTile, n);
        x = a.in + a.off[b]; y = a.out + a.off[b];
        d = a.d[b]; p0 = a.p0[b] & 0xFFFFF;
    }
    if (!on) {
        for (int i = i0 + t; i < i1; i += kFsThreads) y[i] = x[i];
        return;
    }
    fs_taps(hs, t);
    float* p1 = xs;
    float* p0s = xs + kFsPlanePhys;
    for (int t0 = i0; t0 < i1; t0 += kFsTile) { // t0 is even: a multiple of the hop, or of the tile
        const int len = min(kFsTile, i1 - t0);
        const int na = (len + 1) >> 1;          // pairs of outputs
        // staged sample q is x[t0 - 128 + q], of the parity of q: zero outside the clip; the adjoint stages g sin phi
        fs_stage<ADJOINT>(x, n, t0, len, p0, d, p1, p0s, t);
        const int o = kFsPer * t;
        if (o >= na) continue;                  // the whole wave, but for the last one of a ragged tile
        // pair a = o + m: .x is output 2 a from P1[a + u], .y is output 2 a + 1 from P0[a + 1 + u], u = 0..127
        v2f acc[kFsPer];
        fs_hilbert(p1, p0s, hs, t, acc);
        // out = c cos phi -+ H sin phi with the centre sample c = x[i] read again (the adjoint's H already carries the sine)
        const int j0 = 2 * o;                   // the first of this thread's 16 outputs, from t0
        float out[2 * kFsPer];
#pragma unroll
        for (int m = 0; m < kFsPer; ++m) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int j = j0 + 2 * m + e;
                const float hx = e ? acc[m].y : acc[m].x;
                float r = 0.f;
                if (j < len) {
                    const int i = t0 + j;
                    const float c = x[i];
                    float sn, cs;
                    sincospif(fs_phase(p0, d, i), &sn, &cs);
                    r = ADJOINT ? fmaf(c, cs, hx) : fmaf(-hx, sn, c * cs);
                }
                out[2 * m + e] = r;
            }
        }
        float* yo = y + t0 + j0;
        if (j0 + 2 * kFsPer <= len && (((size_t)yo) & 15) == 0) {
#pragma unroll
            for (int v = 0; v < kFsPer / 2; ++v) ((float4*)yo)[v] = make_float4(out[4 * v], out[4 * v + 1], out[4 * v + 2], out[4 * v + 3]);
        } else {
#pragma unroll
            for (int v = 0; v < 2 * kFsPer; ++v)
                if (j0 + v < len) yo[v] = out[v];
        }
    }
}

}  // namespace

void launch_frequency_shift(const ShiftLaunch& L, hipStream_t st) {
    const bool loop = L.draw.frame_off != nullptr;
    auto k = loop ? (L.adjoint ? frequency_shift_kernel<true, true> : frequency_shift_kernel<true, false>)
                  : (L.adjoint ? frequency_shift_kernel<false, true> : frequency_shift_kernel<false, false>);
    hipLaunchKernelGGL(k, stage_grid(L.draw, L.B, L.max_len, kFsTile), dim3(kFsThreads), 0, st, L);
}

}  // namespace aware
