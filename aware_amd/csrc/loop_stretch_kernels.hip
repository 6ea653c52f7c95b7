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
// 256-float clip alignment allows; the stand-alone entry takes any offset and length and stores scalars.
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "kernels.h"
#include "loop_rng.hpp"

namespace aware {

namespace {

constexpr int kStThreads = 256;
constexpr int kStHop = 256, kStWin = 1024;
static_assert(kStHop == kHop && kStHop % 4 == 0, "four consecutive outputs share their frames");

// a_t = (t H Q) >> 16: where segment t of the input starts (its centre, with the window's 512 taken off both sides)
__device__ __forceinline__ long long stretch_pos(long long t, long long Q) { return (t * kStHop * Q) >> 16; }

// z[n0 .. n0 + 3] from x[0 .. n)
__device__ __forceinline__ void stretch_forward4(const float* __restrict__ x, int n, const float* __restrict__ w, long long Q,
                                                 int n0, float v[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.f;
    const int tmax = (n0 + kStWin / 2) / kStHop;              // the last frame whose window holds n0 .. n0 + 3
#pragma unroll
    for (int k = 3; k >= 0; --k) {
        const int t = tmax - k;                               // >= -1
        const int wi = n0 - t * kStHop + kStWin / 2;          // 0 <= wi, wi + 3 < 1024
        const long long src = (long long)(n0 - t * kStHop) + stretch_pos(t, Q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long long s = src + e;
            if (s >= 0 && s < n) v[e] = fmaf(w[wi + e], x[s], v[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] *= 0.5f;
}

// gx[j0 .. j0 + 3] from gz[0 .. n_out)
__device__ __forceinline__ void stretch_adjoint4(const float* __restrict__ gz, int n_out, const float* __restrict__ w,
                                                 long long Q, int j0, float g[4]) {
    g[0] = g[1] = g[2] = g[3] = 0.f;
    // the first t with a_t >= j0 - 511, that is t Q / 256 >= j0 - 511: the ceiling of (j0 - 511) 256 / Q (a division of a
    // negative numerator truncates towards zero, which is its ceiling)
    const long long num = ((long long)j0 - (kStWin / 2 - 1)) * kStHop;
    long long t = num > 0 ? (num + Q - 1) / Q : num / Q;
    if (t < -2) t = -2;
    for (;; ++t) {
        const long long at = stretch_pos(t, Q);
        if (at > (long long)j0 + 3 + kStWin / 2) break;
        const long long wi = (long long)j0 - at + kStWin / 2;         // window index of output j0
        const long long o = (long long)j0 - at + t * kStHop;          // the sample of gz that reaches it
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (wi + e >= 0 && wi + e < kStWin && o + e >= 0 && o + e < n_out) g[e] = fmaf(w[wi + e], gz[o + e], g[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] *= 0.5f;
}

template <bool LOOP>
__global__ __launch_bounds__(kStThreads) void stretch_kernel(StretchLaunch a) {
    __shared__ float s_w[kStWin];
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
    } else {
        nx = a.x_len[b]; nz = a.z_len[b];
        x = a.in + (a.adjoint ? a.z_off[b] : a.x_off[b]);
        y = a.out + (a.adjoint ? a.x_off[b] : a.z_off[b]);
        q0 = blockIdx.x * kStThreads; q1 = q0 + kStThreads;
        m = a.m[b];
        if (m < kStretchMin || m > kStretchMax) m = 0;        // no rate the operator is defined for: the clip is copied
    }
    const int n_in = a.adjoint ? nz : nx, n_w = a.adjoint ? nx : nz;       // samples read / written
    q1 = min(q1, (n_w + 3) / 4);
    if (m != 0) {                                                           // the same for every thread of the workgroup
        for (int i = threadIdx.x; i < kStWin; i += kStThreads) s_w[i] = a.window[i];
        __syncthreads();
    }
    const long long Q = 65536 + (long long)m;
    for (int q = q0 + threadIdx.x; q < q1; q += kStThreads) {
        const int i = 4 * q;
        float v[4];
        if (m == 0) {
            // the identity, exactly (the two sides differ in length only in the stand-alone entry)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = i + e < n_in ? x[i + e] : 0.f;
        } else if (a.adjoint) {
            stretch_adjoint4(x, nz, s_w, Q, i, v);
        } else {
            stretch_forward4(x, nx, s_w, Q, i, v);
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

const float* stretch_window() {
    static std::mutex mu;
    static std::map<int, float*> tables;                      // one per device, kept for the life of the process
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    auto it = tables.find(dev);
    if (it != tables.end()) return it->second;
    const double PI = 3.14159265358979323846;
    std::vector<float> h(kStWin);
    for (int i = 0; i < kStWin; ++i) h[i] = (float)(0.5 - 0.5 * cos(2 * PI * i / kStWin));      // as aware_plan_create's
    float* d = nullptr;
    if (hipMalloc(&d, kStWin * sizeof(float)) != hipSuccess) return nullptr;
    if (hipMemcpy(d, h.data(), kStWin * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return nullptr; }
    tables[dev] = d;
    return d;
}

void launch_time_stretch(const StretchLaunch& L, hipStream_t st) {
    if (L.draw.frame_off) {
        hipLaunchKernelGGL(stretch_kernel<true>, dim3((unsigned)L.draw.pstride, (unsigned)L.B, 1), dim3(kStThreads), 0, st, L);
    } else {
        const unsigned gx = (unsigned)((L.max_len + 4 * kStThreads - 1) / (4 * kStThreads));
        hipLaunchKernelGGL(stretch_kernel<false>, dim3(gx, (unsigned)L.B, 1), dim3(kStThreads), 0, st, L);
    }
}

}  // namespace aware
