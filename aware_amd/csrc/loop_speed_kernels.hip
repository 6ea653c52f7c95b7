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
// with the speed search's views (speed_search_kernels.hip) and the pitch shift; the way in, the identity and the store are
// loop_stage.hpp's, shared with the other stage kernels.
#include "loop_stage.hpp"
#include "speed_interp.hpp"

namespace aware {

namespace {

template <bool LOOP>
__global__ __launch_bounds__(kResampleThreads) void speed_kernel(ResampleLaunch a) {
    const int b = blockIdx.y;
    const float* x;
    float* y;
    int nx, nz, q0, q1, m;          // lengths of the x side and the z side; this workgroup's groups of four outputs [q0, q1)
    LoopStage s;
    if (LOOP && !loop_stage_enter(a.draw, b, s)) return;
    resample_enter<LOOP, true>(a, b, s, x, y, nx, nz, q0, q1, m);
    const int n_in = a.adjoint ? nz : nx, n_w = a.adjoint ? nx : nz;       // samples read / written
    q1 = min(q1, (n_w + 3) / 4);
    const long long R = 65536 + (long long)m;
    for (int q = q0 + threadIdx.x; q < q1; q += kResampleThreads) {
        const int i = 4 * q;
        float v[4];
        if (m == 0) {
            load4(x, n_in, i, v);           // the two sides differ in length only in the stand-alone entry
        } else if (a.adjoint) {
            speed_adjoint4(x, nz, nx, R, i, v);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = speed_tap(x, nx, R, i + e);
        }
        store4<LOOP>(y, n_w, q, v);
    }
}

}  // namespace

void launch_speed_change(const ResampleLaunch& L, hipStream_t st) {
    hipLaunchKernelGGL(L.draw.frame_off ? speed_kernel<true> : speed_kernel<false>, stage_grid(L.draw, L.B, L.max_len, 4 * kResampleThreads),
                       dim3(kResampleThreads), 0, st, L);
}

}  // namespace aware
