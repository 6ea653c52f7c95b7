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
// of u (of gu) that the tile reaches, in groups of four samples, with stretch_kernel's forward (ola.hpp ola_forward4) and
// speed_kernel's adjoint (speed_interp.hpp speed_adjoint4); phase two interpolates (speed_mix) or gathers the frames
// (ola_adjoint4) from LDS.  Every sum keeps the ascending order of the two operators: no atomics,
// one fixed order, and a sample's value does not depend on the tile it is computed for.  m = 0 copies the clip: the identity is
// exact.  Inside the loop one workgroup works through one synthesis run of a clip (the partition chain_kernel uses) with
// float4 stores; the stand-alone entry takes any offset and length and stores scalars.
#include "loop_stage.hpp"
#include "ola.hpp"
#include "speed_interp.hpp"

namespace aware {

namespace {

constexpr int kPsTile = 4 * kResampleThreads;             // outputs of one tile

// forward: the Catmull-Rom taps of outputs i .. i + 1023 lie in u[(i R >> 16) - 1 .. ((i + 1023) R >> 16) + 2]: at most
// ceil(1023 R / 65536) + 4 samples, and up to 3 more in front so that the span starts at a multiple of four
constexpr int kPsSpanFwd = (int)(((long long)(kPsTile - 1) * (65536 + kSpeedMax) + 65535) / 65536) + 4 + 3;
// adjoint: input samples j .. j + 1023 lie in the segments of the frames t with j - 511 <= a_t <= j + 1023 + 512: 2047
// integers, and consecutive a_t are at least floor(256 Q / 65536) apart; frame t reads gu[t H - 512 .. t H + 511]
constexpr int kPsMinStep = (int)(((long long)kOlaHop * (65536 + kStretchMin)) >> 16);
constexpr int kPsFrames = (kPsTile - 1 + kOlaWin - 1) / kPsMinStep + 1;
constexpr int kPsSpanAdj = (kPsFrames - 1) * kOlaHop + kOlaWin + 3;
constexpr int kPsSpan = ((kPsSpanFwd > kPsSpanAdj ? kPsSpanFwd : kPsSpanAdj) + 3) / 4 * 4;
static_assert(kPsSpanFwd == 1296 && kPsFrames == 11 && kPsSpanAdj == 3587 && kPsSpan == 3588, "the spans DESIGN.md section 19 states");
static_assert((kPsSpan + kOlaWin) * sizeof(float) <= 20 * 1024, "the LDS of one workgroup: eight of them share a CU's 160 KiB");
// the coupled rate of every speed offset lies inside the stretch's range: Q = round(2^32 / R)
static_assert(((1ll << 32) + (65536 + kSpeedMax) / 2) / (65536 + kSpeedMax) - 65536 >= kStretchMin &&
              ((1ll << 32) + (65536 + kSpeedMin) / 2) / (65536 + kSpeedMin) - 65536 <= kStretchMax, "");

template <bool LOOP>
__global__ __launch_bounds__(kResampleThreads) void pitch_kernel(ResampleLaunch a) {
    __shared__ float s_w[kOlaWin];
    __shared__ __attribute__((aligned(16))) float s_u[kPsSpan];
    const int b = blockIdx.y;
    const float* x;
    float* y;
    int nx, nz, q0, q1, m;          // lengths of the x side and the z side; this workgroup's groups of four outputs [q0, q1)
    LoopStage s;
    if (LOOP && !loop_stage_enter(a.draw, b, s)) return;
    resample_enter<LOOP>(a, b, s, x, y, nx, nz, q0, q1, m);
    if (m < kSpeedMin || m > kSpeedMax) m = 0;                // no ratio the spans are sized for: the clip is copied
    const int n_in = a.adjoint ? nz : nx, n_w = a.adjoint ? nx : nz;       // samples read / written
    q1 = min(q1, (n_w + 3) / 4);
    if (m == 0) {
        for (int q = q0 + threadIdx.x; q < q1; q += kResampleThreads) {
            float v[4];
            load4(x, n_in, 4 * q, v);       // the two sides differ in length only in the stand-alone entry
            store4<LOOP>(y, n_w, q, v);
        }
        return;
    }
    for (int i = threadIdx.x; i < kOlaWin; i += kResampleThreads) s_w[i] = a.window[i];
    const long long R = 65536 + (long long)m;
    const long long Q = ((1ll << 32) + R / 2) / R;
    const int Lu = nx > 0 ? (int)((((long long)nx - 1) << 16) / Q) + 1 : 0;       // the stretched clip's true length
    // q0, q1, m and everything derived from them are the same for every thread of the workgroup: the barriers are uniform
    for (int qt = q0; qt < q1; qt += kResampleThreads) {
        const int ta = 4 * qt;                                // the tile's first output
        int lo, cnt;                                          // s_u holds u (gu) [lo, lo + cnt)
        if (!a.adjoint) {
            lo = ((int)(((long long)ta * R) >> 16) - 1) & ~3;
            cnt = (int)(((long long)(ta + kPsTile - 1) * R) >> 16) + 2 - lo + 1;
        } else {
            long long slo = 0x7FFFFFFF, shi = -1;
            for (long long t = ola_first_frame(ta, Q);; ++t) {
                const long long at = ola_pos(t, Q);
                if (at > (long long)ta + kPsTile - 1 + kOlaWin / 2) break;
                slo = min(slo, max((long long)ta - at, -(long long)(kOlaWin / 2)) + t * kOlaHop);
                shi = max(shi, min((long long)ta + kPsTile - 1 - at, (long long)(kOlaWin / 2 - 1)) + t * kOlaHop);
            }
            slo = max(slo, 0ll); shi = min(shi, (long long)Lu - 1);
            lo = (int)slo & ~3;
            cnt = shi >= slo ? (int)(shi - lo + 1) : 0;
        }
        cnt = min(cnt, kPsSpan);                              // the static bounds above: never binds
        __syncthreads();                                      // the window is staged; the last tile's reads of s_u are done
        for (int g = threadIdx.x; 4 * g < cnt; g += kResampleThreads) {
            const int k0 = lo + 4 * g;                        // >= 0 in the adjoint
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (!a.adjoint) {
                ola_forward4<true>(x, nx, s_w, Q, Lu, k0, v);
            } else if (k0 < Lu) {                             // the resampling of u[0 .. Lu) transposed; zero from Lu on
                speed_adjoint4(x, nz, Lu, R, k0, v);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k0 + e >= Lu) v[e] = 0.f;
            }
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
                if (p <= plim && k + 3 < cnt) v[e] = speed_mix(speed_weights_at(p), s_u[k], s_u[k + 1], s_u[k + 2], s_u[k + 3]);
            }
        } else {
            ola_adjoint4(s_u, cnt, lo, s_w, Q, i, v);
        }
        store4<LOOP>(y, n_w, q, v);
    }
}

}  // namespace

void launch_pitch_shift(const ResampleLaunch& L, hipStream_t st) {
    hipLaunchKernelGGL(L.draw.frame_off ? pitch_kernel<true> : pitch_kernel<false>, stage_grid(L.draw, L.B, L.max_len, kPsTile),
                       dim3(kResampleThreads), 0, st, L);
}

}  // namespace aware
