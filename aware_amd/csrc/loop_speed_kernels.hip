// Speed change (EXTENSION, parity unpinned: the reference has neither the attack nor a chain inside its loop): the clip
// played at the ratio R / 65536, R = 65536 + m, through Catmull-Rom interpolation.  DESIGN.md section 17; the torch
// restatement is aware_amd/embedding/loop_attacks.py::speed_change / apply_chain.
//
//   r = philox4x32_10((0, s, 1 + j, 1), (seed_b, 0x5EED)),  on = (r0 + 0.5) / 2^32 < prob,
//   m = m_lo + ((r3 * (m_hi - m_lo + 1)) >> 32),  R = 65536 + m          (m = 0 where the entry does not fire, and behind a
//   phase vocoder that drew its stretch mode: `coin`)
//   p_i = i R (64-bit, 16.16 fixed point),  i0 = p_i >> 16,  f = (p_i & 0xFFFF) / 65536   (exact in f32)
//   forward   z[i] = w_-1(f) x[i0 - 1] + w_0(f) x[i0] + w_1(f) x[i0 + 1] + w_2(f) x[i0 + 2],  x zero outside [0, n),
//             z[i] = 0 where p_i > (n - 1) << 16
//   adjoint   gx[j] = sum over ascending i of w_{j - i0(i)}(f_i) gy[i],  i from ceil(((j - 2) << 16) / R) while i0(i) <= j + 1
//
// One kernel for both directions and both layouts; every thread owns four consecutive outputs.  The forward gathers its four
// taps per output, the adjoint walks the at most ten inputs that can reach its four outputs, in ascending order: no atomics,
// one fixed order.  m = 0 copies the clip: the identity is exact.  Inside the loop one workgroup works through one synthesis
// run of a clip (the partition chain_kernel uses) with float4 stores, which the 256-float clip alignment allows; the
// stand-alone entry takes any offset and length and stores scalars.  The weights and the tap are speed_interp.hpp's, shared
// with the speed search's views (speed_search_kernels.hip).
#include "common.hpp"
#include "kernels.h"
#include "loop_rng.hpp"
#include "speed_interp.hpp"

namespace aware {

namespace {

constexpr int kSpThreads = 256;

// gx[j0 .. j0 + 3] from gy[0 .. n_out): x has n samples
__device__ __forceinline__ void speed_adjoint4(const float* __restrict__ gy, int n_out, int n, long long R, int j0, float g[4]) {
    g[0] = g[1] = g[2] = g[3] = 0.f;
    const long long lo = ((long long)j0 - 2) << 16, plim = (long long)(n - 1) << 16;
    int i = lo <= 0 ? 0 : (int)(((unsigned long long)lo + (unsigned long long)R - 1ull) / (unsigned long long)R);
    for (; i < n_out; ++i) {
        const long long p = (long long)i * R;
        const int i0 = (int)(p >> 16);
        if (p > plim || i0 > j0 + 4) break;
        const SpeedWeights w = speed_weights((float)(unsigned)(p & 0xFFFF) * (1.0f / 65536.0f));
        const float v = gy[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int t = j0 + e - i0;
            const float wt = t == -1 ? w.wm1 : (t == 0 ? w.w0 : (t == 1 ? w.w1 : w.w2));
            if (t >= -1 && t <= 2) g[e] = fmaf(wt, v, g[e]);
        }
    }
}

template <bool LOOP>
__global__ __launch_bounds__(kSpThreads) void speed_kernel(SpeedLaunch a) {
    const int b = blockIdx.y;
    const float* x;
    float* y;
    int nx, nz, q0, q1, m;          // lengths of the x side and the z side; this workgroup's groups of four outputs [q0, q1)
    if (LOOP) {
        if (loop_gate_skips(a.draw.gate, b)) return;
        const int nblk = a.draw.frame_off[b + 1] - a.draw.frame_off[b] - 1;
        int nseg, jb0, jb1;
        synth_segment(nblk, blockIdx.x, a.draw.run_blocks, nseg, jb0, jb1);
        if ((int)blockIdx.x >= nseg) return;
        const int so = sig_offset(a.draw.frame_off, b);
        x = a.in + so; y = a.out + so;
        nx = nz = kHop * nblk;
        q0 = jb0 * (kHop / 4); q1 = jb1 * (kHop / 4);
        unsigned r[4];
        const bool on = loop_entry_draw(a.draw, b, r);
        m = on ? a.m_lo + (int)(((unsigned long long)r[3] * (unsigned long long)(unsigned)(a.m_hi - a.m_lo + 1)) >> 32) : 0;
        if (a.coin && r[2] < 0x80000000u) m = 0;          // behind a phase vocoder in stretch mode: the identity
    } else {
        nx = a.x_len[b]; nz = a.z_len[b];
        x = a.in + (a.adjoint ? a.z_off[b] : a.x_off[b]);
        y = a.out + (a.adjoint ? a.x_off[b] : a.z_off[b]);
        q0 = blockIdx.x * kSpThreads; q1 = q0 + kSpThreads;
        m = a.m[b];
    }
    const int n_in = a.adjoint ? nz : nx, n_w = a.adjoint ? nx : nz;       // samples read / written
    q1 = min(q1, (n_w + 3) / 4);
    const long long R = 65536 + (long long)m;
    for (int q = q0 + threadIdx.x; q < q1; q += kSpThreads) {
        const int i = 4 * q;
        float v[4];
        if (m == 0) {
            // the identity, exactly (the two sides differ in length only in the stand-alone entry)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = i + e < n_in ? x[i + e] : 0.f;
        } else if (a.adjoint) {
            speed_adjoint4(x, nz, nx, R, i, v);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = speed_tap(x, nx, R, i + e);
        }
        if (LOOP) {
            reinterpret_cast<float4*>(y)[q] = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i + e < n_w) y[i + e] = v[e];
        }
    }
}

}  // namespace

void launch_speed_change(const SpeedLaunch& L, hipStream_t st) {
    if (L.draw.frame_off) {
        hipLaunchKernelGGL(speed_kernel<true>, dim3((unsigned)L.draw.pstride, (unsigned)L.B, 1), dim3(kSpThreads), 0, st, L);
    } else {
        const unsigned gx = (unsigned)((L.max_len + 4 * kSpThreads - 1) / (4 * kSpThreads));
        hipLaunchKernelGGL(speed_kernel<false>, dim3(gx, (unsigned)L.B, 1), dim3(kSpThreads), 0, st, L);
    }
}

}  // namespace aware
