// Pitch shift (EXTENSION, parity unpinned: the reference's PitchShift is a library call, and it has no chain inside its
// loop): the clip's pitch moved by the ratio R / 65536, R = 65536 + m, at its own duration, as the speed change of the
// overlap-add stretch at the coupled rate.  DESIGN.md section 19; the torch restatement is
// aware_amd/embedding/loop_attacks.py::pitch_shift / apply_chain.
//
//   r = philox4x32_10((0, s, 1 + j, 1), (seed_b, 0x5EED)),  on = (r0 + 0.5) / 2^32 < prob,
//   m = m_lo + ((r3 * (m_hi - m_lo + 1)) >> 32),  R = 65536 + m          (m = 0 where the entry does not fire)
//   Q = (2^32 + R / 2) / R (64-bit),  L_u = ((n - 1) << 16) / Q + 1,  a_t = (t H Q) >> 16,  p_i = i R
//   forward   u[k] = 1/2 sum over ascending t of w[k - t H + 512] x[k - t H + a_t]  for 0 <= k < L_u, zero elsewhere
//             z[i] = w_-1(f) u[i0 - 1] + w_0(f) u[i0] + w_1(f) u[i0 + 1] + w_2(f) u[i0 + 2],  i0 = p_i >> 16,
//             f = (p_i & 0xFFFF) / 65536,  z[i] = 0 where p_i > (L_u - 1) << 16
//   adjoint   gu[k] = sum over ascending i of w_{k - i0(i)}(f_i) gz[i]  for 0 <= k < L_u, zero elsewhere
//             gx[j] = 1/2 sum over ascending t of w[j - a_t + 512] gu[j - a_t + t H]
//
// u has another length than the clip, so it never exists in memory: one kernel for both directions and both layouts works
// through its outputs in tiles of 1024 (four per thread), and per tile in two phases through LDS.  Phase one computes the span
// of u (of gu) that the tile reaches, in groups of four samples as stretch_kernel's forward (speed_kernel's adjoint) does;
// phase two interpolates (gathers the frames) from LDS.  Every sum keeps the ascending order of the two operators: no atomics,
// one fixed order, and a sample's value does not depend on the tile it is computed for.  m = 0 copies the clip: the identity is
// exact.  Inside the loop one workgroup works through one synthesis run of a clip (the partition chain_kernel uses) with
// float4 stores; the stand-alone entry takes any offset and length and stores scalars.
#include "common.hpp"
#include "kernels.h"
#include "loop_rng.hpp"

namespace aware {

namespace {

constexpr int kPsThreads = 256;
constexpr int kPsTile = 4 * kPsThreads;                   // outputs of one tile
constexpr int kPsHop = 256, kPsWin = 1024;                // the stretch's geometry (loop_stretch_kernels.hip)
static_assert(kPsHop == kHop && kPsHop % 4 == 0, "four consecutive samples of u share their frames");

// forward: the Catmull-Rom taps of outputs i .. i + 1023 lie in u[(i R >> 16) - 1 .. ((i + 1023) R >> 16) + 2]: at most
// ceil(1023 R / 65536) + 4 samples, and up to 3 more in front so that the span starts at a multiple of four
constexpr int kPsSpanFwd = (int)(((long long)(kPsTile - 1) * (65536 + kSpeedMax) + 65535) / 65536) + 4 + 3;
// adjoint: input samples j .. j + 1023 lie in the segments of the frames t with j - 511 <= a_t <= j + 1023 + 512: 2047
// integers, and consecutive a_t are at least floor(256 Q / 65536) apart; frame t reads gu[t H - 512 .. t H + 511]
constexpr int kPsMinStep = (int)(((long long)kPsHop * (65536 + kStretchMin)) >> 16);
constexpr int kPsFrames = (kPsTile - 1 + kPsWin - 1) / kPsMinStep + 1;
constexpr int kPsSpanAdj = (kPsFrames - 1) * kPsHop + kPsWin + 3;
constexpr int kPsSpan = ((kPsSpanFwd > kPsSpanAdj ? kPsSpanFwd : kPsSpanAdj) + 3) / 4 * 4;
static_assert(kPsSpanFwd == 1296 && kPsFrames == 11 && kPsSpanAdj == 3587 && kPsSpan == 3588, "the spans DESIGN.md section 19 states");
static_assert((kPsSpan + kPsWin) * sizeof(float) <= 20 * 1024, "the LDS of one workgroup: eight of them share a CU's 160 KiB");
// the coupled rate of every speed offset lies inside the stretch's range: Q = round(2^32 / R)
static_assert(((1ll << 32) + (65536 + kSpeedMax) / 2) / (65536 + kSpeedMax) - 65536 >= kStretchMin &&
              ((1ll << 32) + (65536 + kSpeedMin) / 2) / (65536 + kSpeedMin) - 65536 <= kStretchMax, "");

struct PitchWeights { float wm1, w0, w1, w2; };

// the Horner form of speed_kernel, in explicit fused multiply-adds, so that every instantiation rounds the same way
__device__ __forceinline__ PitchWeights pitch_weights(float f) {
    PitchWeights w;
    w.wm1 = (fmaf(2.f - f, f, -1.f) * f) * 0.5f;              // ((-f + 2) f - 1) f / 2
    w.w0 = fmaf(fmaf(3.f, f, -5.f), f * f, 2.f) * 0.5f;       // ((3 f - 5) f^2 + 2) / 2
    w.w1 = (fmaf(fmaf(-3.f, f, 4.f), f, 1.f) * f) * 0.5f;     // ((-3 f + 4) f + 1) f / 2
    w.w2 = ((f - 1.f) * (f * f)) * 0.5f;                      // (f - 1) f^2 / 2
    return w;
}

// a_t = (t H Q) >> 16: where segment t of the input starts
__device__ __forceinline__ long long pitch_pos(long long t, long long Q) { return (t * kPsHop * Q) >> 16; }

// u[k0 .. k0 + 3] from x[0 .. n), k0 a multiple of four: the four windowed reads in ascending t, then the halving; zero
// outside [0, Lu)
__device__ __forceinline__ void pitch_stretch4(const float* __restrict__ x, int n, const float* __restrict__ w, long long Q,
                                               int Lu, int k0, float v[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (k0 < 0 || k0 >= Lu) return;
    const int tmax = (k0 + kPsWin / 2) / kPsHop;              // the last frame whose window holds k0 .. k0 + 3
#pragma unroll
    for (int k = 3; k >= 0; --k) {
        const int t = tmax - k;                               // >= -1
        const int wi = k0 - t * kPsHop + kPsWin / 2;          // 0 <= wi, wi + 3 < 1024
        const long long src = (long long)(k0 - t * kPsHop) + pitch_pos(t, Q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long long s = src + e;
            if (s >= 0 && s < n) v[e] = fmaf(w[wi + e], x[s], v[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = k0 + e < Lu ? v[e] * 0.5f : 0.f;
}

// gu[k0 .. k0 + 3] from gz[0 .. n_out), k0 >= 0: the resampling of u[0 .. Lu) transposed, over ascending i; zero from Lu on
__device__ __forceinline__ void pitch_resample_adjoint4(const float* __restrict__ gz, int n_out, int Lu, long long R, int k0,
                                                        float g[4]) {
    g[0] = g[1] = g[2] = g[3] = 0.f;
    if (k0 >= Lu) return;
    const long long lo = ((long long)k0 - 2) * 65536, plim = ((long long)Lu - 1) * 65536;
    int i = lo <= 0 ? 0 : (int)(((unsigned long long)lo + (unsigned long long)R - 1ull) / (unsigned long long)R);
    for (; i < n_out; ++i) {
        const long long p = (long long)i * R;
        const int i0 = (int)(p >> 16);
        if (p > plim || i0 > k0 + 4) break;
        const PitchWeights w = pitch_weights((float)(unsigned)(p & 0xFFFF) * (1.0f / 65536.0f));
        const float v = gz[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int t = k0 + e - i0;
            const float wt = t == -1 ? w.wm1 : (t == 0 ? w.w0 : (t == 1 ? w.w1 : w.w2));
            if (t >= -1 && t <= 2) g[e] = fmaf(wt, v, g[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (k0 + e >= Lu) g[e] = 0.f;
}

// the first frame t >= -2 with a_t >= j - 511: the ceiling of (j - 511) 256 / Q (a division of a negative numerator truncates
// towards zero, which is its ceiling)
__device__ __forceinline__ long long pitch_first_frame(int j, long long Q) {
    const long long num = ((long long)j - (kPsWin / 2 - 1)) * kPsHop;
    const long long t = num > 0 ? (num + Q - 1) / Q : num / Q;
    return t < -2 ? -2 : t;
}

template <bool LOOP>
__global__ __launch_bounds__(kPsThreads) void pitch_kernel(PitchLaunch a) {
    __shared__ float s_w[kPsWin];
    __shared__ __attribute__((aligned(16))) float s_u[kPsSpan];
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
        q0 = blockIdx.x * kPsThreads; q1 = q0 + kPsThreads;
        m = a.m[b];
    }
    if (m < kSpeedMin || m > kSpeedMax) m = 0;                // no ratio the spans are sized for: the clip is copied
    const int n_in = a.adjoint ? nz : nx, n_w = a.adjoint ? nx : nz;       // samples read / written
    q1 = min(q1, (n_w + 3) / 4);
    if (m == 0) {
        // the identity, exactly (the two sides differ in length only in the stand-alone entry)
        for (int q = q0 + threadIdx.x; q < q1; q += kPsThreads) {
            const int i = 4 * q;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = i + e < n_in ? x[i + e] : 0.f;
            if (LOOP) {
                reinterpret_cast<float4*>(y)[q] = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (i + e < n_w) y[i + e] = v[e];
            }
        }
        return;
    }
    for (int i = threadIdx.x; i < kPsWin; i += kPsThreads) s_w[i] = a.window[i];
    const long long R = 65536 + (long long)m;
    const long long Q = ((1ll << 32) + R / 2) / R;
    const int Lu = nx > 0 ? (int)((((long long)nx - 1) << 16) / Q) + 1 : 0;       // the stretched clip's true length
    // q0, q1, m and everything derived from them are the same for every thread of the workgroup: the barriers are uniform
    for (int qt = q0; qt < q1; qt += kPsThreads) {
        const int ta = 4 * qt;                                // the tile's first output
        int lo, cnt;                                          // s_u holds u (gu) [lo, lo + cnt)
        if (!a.adjoint) {
            lo = ((int)(((long long)ta * R) >> 16) - 1) & ~3;
            cnt = (int)(((long long)(ta + kPsTile - 1) * R) >> 16) + 2 - lo + 1;
        } else {
            long long slo = 0x7FFFFFFF, shi = -1;
            for (long long t = pitch_first_frame(ta, Q);; ++t) {
                const long long at = pitch_pos(t, Q);
                if (at > (long long)ta + kPsTile - 1 + kPsWin / 2) break;
                slo = min(slo, max((long long)ta - at, -(long long)(kPsWin / 2)) + t * kPsHop);
                shi = max(shi, min((long long)ta + kPsTile - 1 - at, (long long)(kPsWin / 2 - 1)) + t * kPsHop);
            }
            slo = max(slo, 0ll); shi = min(shi, (long long)Lu - 1);
            lo = (int)slo & ~3;
            cnt = shi >= slo ? (int)(shi - lo + 1) : 0;
        }
        cnt = min(cnt, kPsSpan);                              // the static bounds above: never binds
        __syncthreads();                                      // the window is staged; the last tile's reads of s_u are done
        for (int g = threadIdx.x; 4 * g < cnt; g += kPsThreads) {
            float v[4];
            if (a.adjoint) pitch_resample_adjoint4(x, nz, Lu, R, lo + 4 * g, v);
            else pitch_stretch4(x, nx, s_w, Q, Lu, lo + 4 * g, v);
            *reinterpret_cast<float4*>(s_u + 4 * g) = make_float4(v[0], v[1], v[2], v[3]);
        }
        __syncthreads();
        const int q = qt + threadIdx.x;
        if (q >= q1) continue;
        const int i = 4 * q;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (!a.adjoint) {
            const long long plim = ((long long)Lu - 1) * 65536;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long long p = (long long)(i + e) * R;
                const int k = (int)(p >> 16) - 1 - lo;        // >= 0: lo is at most the first output's i0 - 1
                if (p <= plim && k + 3 < cnt) {
                    const PitchWeights w = pitch_weights((float)(unsigned)(p & 0xFFFF) * (1.0f / 65536.0f));
                    v[e] = fmaf(w.w2, s_u[k + 3], fmaf(w.w1, s_u[k + 2], fmaf(w.w0, s_u[k + 1], w.wm1 * s_u[k])));
                }
            }
        } else {
            for (long long t = pitch_first_frame(i, Q);; ++t) {
                const long long at = pitch_pos(t, Q);
                if (at > (long long)i + 3 + kPsWin / 2) break;
                const long long wi = (long long)i - at + kPsWin / 2;          // window index of output i
                const long long o = (long long)i - at + t * kPsHop - lo;      // the sample of gu that reaches it, in s_u
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (wi + e >= 0 && wi + e < kPsWin && o + e >= 0 && o + e < cnt) v[e] = fmaf(s_w[wi + e], s_u[o + e], v[e]);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= 0.5f;
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

void launch_pitch_shift(const PitchLaunch& L, hipStream_t st) {
    if (L.draw.frame_off) {
        hipLaunchKernelGGL(pitch_kernel<true>, dim3((unsigned)L.draw.pstride, (unsigned)L.B, 1), dim3(kPsThreads), 0, st, L);
    } else {
        const unsigned gx = (unsigned)((L.max_len + kPsTile - 1) / kPsTile);
        hipLaunchKernelGGL(pitch_kernel<false>, dim3(gx, (unsigned)L.B, 1), dim3(kPsThreads), 0, st, L);
    }
}

}  // namespace aware
