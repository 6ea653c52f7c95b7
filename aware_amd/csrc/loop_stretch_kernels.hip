// Time stretch (EXTENSION, parity unpinned: the reference's TimeStretch is rubberband, and it has no chain inside its loop):
// the clip's duration divided by Q / 65536, Q = 65536 + m, at its own pitch, by plain overlap-add of Hann-windowed segments.
// DESIGN.md section 18; the torch restatement is aware_amd/embedding/loop_attacks.py::time_stretch / apply_chain.
//
//   r = philox4x32_10((0, s, 1 + j, 1), (seed_b, 0x5EED)),  on = (r0 + 0.5) / 2^32 < prob,
//   m = m_lo + ((r3 * (m_hi - m_lo + 1)) >> 32),  Q = 65536 + m          (m = 0 where the entry does not fire)
//   H = 256, N = 1024, w the periodic Hann window of N points in f32,  a_t = (t H Q) >> 16 (64-bit, arithmetic) for t >= -2
//   forward   z[n]  = 1/2 sum over ascending t of w[n - t H + 512] x[n - t H + a_t],   0 <= n - t H + 512 < N (four t),
//             x zero outside [0, n_in)
//   adjoint   gx[j] = 1/2 sum over ascending t of w[j - a_t + 512] gz[j - a_t + t H],  0 <= j - a_t + 512 < N (at most six t),
//             gz zero outside [0, n_out)
//
// One kernel for both directions and both layouts; every thread owns four consecutive outputs, which share their frames: the
// forward's four t are those of the hop the outputs lie in, the adjoint walks the at most seven t whose segment reaches one of
// its four outputs, in ascending order: no atomics, one fixed order.  The window is a table of 1024 floats computed on the
// host as the plan's is (stretch_window) and staged in LDS.  m = 0 copies the clip: the identity is exact.  Inside the loop
// one workgroup works through one synthesis run of a clip (the partition chain_kernel uses) with float4 stores, which the
// 256-float clip alignment allows; the stand-alone entry takes any offset and length and stores scalars.  The two sums are
// ola.hpp's, shared with the pitch shift; the way in, the identity and the store are loop_stage.hpp's.
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "loop_stage.hpp"
#include "ola.hpp"

namespace aware {

namespace {

template <bool LOOP>
__global__ __launch_bounds__(kResampleThreads) void stretch_kernel(ResampleLaunch a) {
    __shared__ float s_w[kOlaWin];
    const int b = blockIdx.y;
    const float* x;
    float* y;
    int nx, nz, q0, q1, m;          // lengths of the x side and the z side; this workgroup's groups of four outputs [q0, q1)
    LoopStage s;
    if (LOOP && !loop_stage_enter(a.draw, b, s)) return;
    resample_enter<LOOP>(a, b, s, x, y, nx, nz, q0, q1, m);
    if (!LOOP && (m < kStretchMin || m > kStretchMax)) m = 0;               // no rate the operator is defined for: the clip is copied
    const int n_in = a.adjoint ? nz : nx, n_w = a.adjoint ? nx : nz;       // samples read / written
    q1 = min(q1, (n_w + 3) / 4);
    if (m != 0) {                                                           // the same for every thread of the workgroup
        for (int i = threadIdx.x; i < kOlaWin; i += kResampleThreads) s_w[i] = a.window[i];
        __syncthreads();
    }
    const long long Q = 65536 + (long long)m;
    for (int q = q0 + threadIdx.x; q < q1; q += kResampleThreads) {
        const int i = 4 * q;
        float v[4];
        if (m == 0) {
            load4(x, n_in, i, v);           // the two sides differ in length only in the stand-alone entry
        } else if (a.adjoint) {
            ola_adjoint4(x, nz, 0, s_w, Q, i, v);
        } else {
            ola_forward4<false>(x, nx, s_w, Q, 0, i, v);
        }
        store4<LOOP>(y, n_w, q, v);
    }
}

}  // namespace

const float* stretch_window() {
    static std::mutex mu;
    static std::map<int, float*> tables;                      // one per device, kept for the life of the process
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    auto it = tables.find(dev);
    if (it != tables.end()) return it->second;
    const double PI = 3.14159265358979323846;
    std::vector<float> h(kOlaWin);
    for (int i = 0; i < kOlaWin; ++i) h[i] = (float)(0.5 - 0.5 * cos(2 * PI * i / kOlaWin));      // as aware_plan_create's
    float* d = nullptr;
    if (hipMalloc(&d, kOlaWin * sizeof(float)) != hipSuccess) return nullptr;
    if (hipMemcpy(d, h.data(), kOlaWin * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return nullptr; }
    tables[dev] = d;
    return d;
}

void launch_time_stretch(const ResampleLaunch& L, hipStream_t st) {
    hipLaunchKernelGGL(L.draw.frame_off ? stretch_kernel<true> : stretch_kernel<false>, stage_grid(L.draw, L.B, L.max_len, 4 * kResampleThreads),
                       dim3(kResampleThreads), 0, st, L);
}

}  // namespace aware
