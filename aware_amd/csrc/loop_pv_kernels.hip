// Phase vocoder inside the embed loop (EXTENSION, parity unpinned: the reference has neither the attack nor a chain inside its
// loop): the frames of a clip's spectrum resampled in time at the rate Q / 65536, magnitudes interpolated between the two
// neighbouring frames, phases accumulated as a product of unit phasors.  DESIGN.md section 20; the torch restatement is
// aware_amd/embedding/loop_attacks.py::pv_frames / pv_stretch / apply_chain.
//
//   r = philox4x32_10((0, s, 1 + j, 1), (seed_b, 0x5EED)),  on = (r0 + 0.5) / 2^32 < prob
//   stretch mode (the only mode with q_lo <= q_hi alone; with both ranges where r2 < 2^31):
//       mq = q_lo + ((r3 * (q_hi - q_lo + 1)) >> 32),  m = 0
//   pitch mode:  m = m_lo + ((r3 * (m_hi - m_lo + 1)) >> 32),  R = 65536 + m,  mq = ((1 << 32) + R / 2) / R - 65536
//   Q = 65536 + mq;  for t < T:  p = t Q (64-bit),  i = p >> 16,  al = (p & 0xFFFF) / 65536   (exact in f32)
//   forward   Y[t] = ((1 - al) |S[i]| + al |S[i + 1]|) P[t],  S[T] := 0,  Y[t] = 0 where i >= T
//             P[0] = u(S[0]),  P[t + 1] = P[t] u(S[i + 1]) conj(u(S[i])),  u(c) = c / |c|, u(c) = 1 where Re c == 0 and Im c == 0
//   backward  gm[t] = Re(conj(P[t]) G[t]);  gmag[i] += (1 - al) gm[t],  gmag[i + 1] += al gm[t] over ascending t;
//             gS[i] = gmag[i] u(S[i]), 0 where S[i] is a zero cell (d|c|/dc at 0);  P and Q are constants
//
// One thread per clip and bin, sequential over the clip's T output frames in f32; rows are 520 complex wide, so a wave reads 64
// adjacent bins of a frame.  The source index is monotone and advances by at most 2 per frame (Q / 65536 <= 4/3): S[i] and
// S[i + 1] stay in registers as (|c|, u(c)), the two frames behind them are in flight, every source frame is loaded once, and
// every load is guarded by its row < T.  The backward pass recomputes P with the forward's recurrence, keeps gmag[i] and
// gmag[i + 1] in registers and flushes a row when i leaves it: no atomics, no LDS, one fixed order.  gS may be S itself (a row is
// written after it has been read); it is never G.  P is pulled back to the unit circle by one Newton step per frame.
#include "common.hpp"
#include "kernels.h"
#include "loop_stage.hpp"

namespace aware {

namespace {

constexpr int kPvThreads = 64;
constexpr int kPvRow = 520;

// |c|, u(c) and whether c is a non-zero cell.  Scaled by the larger part, so that no square underflows; u of a real cell is
// exactly +-1
struct PvCell { float mag, ux, uy, live; };
__device__ __forceinline__ PvCell pv_cell(cf c) {
    const float s = fmaxf(fabsf(c.x), fabsf(c.y));
    const bool z = s == 0.f;                       // the zero test: both parts compare equal to 0
    const float sd = z ? 1.f : s;
    const float xs = c.x / sd, ys = c.y / sd;
    const float h = z ? 1.f : sqrtf(fmaf(xs, xs, ys * ys));
    PvCell o;
    o.mag = z ? 0.f : s * h; o.ux = z ? 1.f : xs / h; o.uy = ys / h; o.live = z ? 0.f : 1.f;
    return o;
}

// row r of the clip's column, the zero frame from row T on: every load is guarded
__device__ __forceinline__ cf pv_load(const cf* S, int r, int T) {
    cf v = mk(0.f, 0.f);
    if (r < T) v = S[(size_t)r * kPvRow];
    return v;
}

// P <- P u(c1) conj(u(c0)), then one Newton step of 1 / |P| at 1
__device__ __forceinline__ void pv_advance(float& px, float& py, const PvCell& c0, const PvCell& c1) {
    const float wx = fmaf(c1.ux, c0.ux, c1.uy * c0.uy), wy = fmaf(c1.uy, c0.ux, -(c1.ux * c0.uy));
    const float nx = fmaf(px, wx, -(py * wy)), ny = fmaf(px, wy, py * wx);
    const float s = fmaf(-0.5f, fmaf(nx, nx, ny * ny), 1.5f);
    px = nx * s; py = ny * s;
}

// the clip's draw: true where the entry fires and moves the clip (mq != 0; pitch mode has mq == 0 exactly where m == 0)
template <bool LOOP>
__device__ __forceinline__ bool pv_draw(const PvLaunch& a, int b, int& mq) {
    if (!LOOP) {
        mq = a.mq[b];
        if (mq < kStretchMin || mq > kStretchMax) mq = 0;
        return true;
    }
    unsigned r[4];
    const bool on = loop_entry_draw(a.draw, b, r);
    const bool has_q = a.q_lo <= a.q_hi, has_m = a.m_lo <= a.m_hi;
    if (has_q && (!has_m || r[2] < 0x80000000u)) {
        mq = loop_uniform(r[3], a.q_lo, a.q_hi);
    } else {
        const int m = loop_uniform(r[3], a.m_lo, a.m_hi);
        const long long R = 65536 + (long long)m;
        mq = (int)(((1ll << 32) + R / 2) / R) - 65536;
    }
    return on && mq != 0;
}

// BWD false: out = Y from spec = S.  BWD true: out = gS from spec = S and grad = G (out may be spec)
template <bool LOOP, bool BWD>
__global__ __launch_bounds__(kPvThreads) void pv_frames_kernel(PvLaunch a) {
    const int b = blockIdx.y, k = blockIdx.x * kPvThreads + threadIdx.x;
    if (k >= kPvRow) return;
    const int f0 = a.draw.frame_off[b], T = a.draw.frame_off[b + 1] - f0;
    if (T < 1) return;
    if (LOOP && loop_gate_skips(a.draw.gate, b)) return;
    int mq;
    const bool on = pv_draw<LOOP>(a, b, mq);
    if (LOOP && !on) return;                       // the clip does not go through the spectra at all (pv_idle_kernel)
    const cf* S = (const cf*)a.spec + (size_t)f0 * kPvRow + k;
    const cf* G = BWD ? (const cf*)a.grad + (size_t)f0 * kPvRow + k : nullptr;
    cf* O = (cf*)a.out + (size_t)f0 * kPvRow + k;
    if (k > 512) {                                 // the 7 pad columns of the 520-wide rows
        for (int t = 0; t < T; ++t) O[(size_t)t * kPvRow] = mk(0.f, 0.f);
        return;
    }
    if (mq == 0) {                                 // the identity, exactly (stand-alone entries only)
        const cf* I = BWD ? G : S;
        for (int t = 0; t < T; ++t) O[(size_t)t * kPvRow] = I[(size_t)t * kPvRow];
        return;
    }
    const long long Q = 65536 + (long long)mq;
    const cf zero = mk(0.f, 0.f);
    int i = 0;
    PvCell c0 = pv_cell(S[0]);
    PvCell c1 = pv_cell(pv_load(S, 1, T));
    cf n0 = pv_load(S, 2, T), n1 = pv_load(S, 3, T);       // S[i + 2], S[i + 3]
    float px = c0.ux, py = c0.uy;
    float g0 = 0.f, g1 = 0.f;                      // gmag[i], gmag[i + 1]
    for (int t = 0; t < T; ++t) {
        const long long p = (long long)t * Q;
        const int it = (int)(p >> 16);
        if (it >= T) {                             // past the end of the clip: zeros from here on
            if (BWD) break;
            O[(size_t)t * kPvRow] = zero;
            continue;
        }
        while (i < it) {
            if (BWD) { O[(size_t)i * kPvRow] = mk(g0 * c0.ux * c0.live, g0 * c0.uy * c0.live); g0 = g1; g1 = 0.f; }
            c0 = c1; c1 = pv_cell(n0); n0 = n1;
            n1 = pv_load(S, i + 4, T);
            ++i;
        }
        const float al = (float)(unsigned)(p & 0xFFFF) * (1.0f / 65536.0f);
        if (BWD) {
            const cf g = G[(size_t)t * kPvRow];
            const float gm = fmaf(px, g.x, py * g.y);
            g0 = fmaf(1.f - al, gm, g0);
            g1 = fmaf(al, gm, g1);
        } else {
            const float mag = fmaf(al, c1.mag, (1.f - al) * c0.mag);
            O[(size_t)t * kPvRow] = mk(mag * px, mag * py);
        }
        pv_advance(px, py, c0, c1);
    }
    if (BWD) {
        O[(size_t)i * kPvRow] = mk(g0 * c0.ux * c0.live, g0 * c0.uy * c0.live);
        if (i + 1 < T) O[(size_t)(i + 1) * kPvRow] = mk(g1 * c1.ux * c1.live, g1 * c1.uy * c1.live);
        for (int r = i + 2; r < T; ++r) O[(size_t)r * kPvRow] = zero;
    }
}

// A clip that the entry leaves alone at this step: dst = src, so that it never sees the spectra (one workgroup per synthesis
// run, as speed_kernel)
__global__ __launch_bounds__(256) void pv_idle_kernel(PvLaunch a, const float* __restrict__ src, float* __restrict__ dst) {
    const int b = blockIdx.y;
    if (loop_gate_skips(a.draw.gate, b)) return;
    const int nblk = a.draw.frame_off[b + 1] - a.draw.frame_off[b] - 1;
    int nseg, jb0, jb1;
    synth_segment(nblk, blockIdx.x, a.draw.run_blocks, nseg, jb0, jb1);
    if ((int)blockIdx.x >= nseg) return;
    int mq;
    if (pv_draw<true>(a, b, mq)) return;
    const int so = sig_offset(a.draw.frame_off, b);
    const float4* s4 = reinterpret_cast<const float4*>(src + so);
    float4* d4 = reinterpret_cast<float4*>(dst + so);
    for (int q = jb0 * (kHop / 4) + threadIdx.x; q < jb1 * (kHop / 4); q += 256) d4[q] = s4[q];
}

}  // namespace

void launch_pv_frames(const PvLaunch& L, int backward, hipStream_t st) {
    const dim3 grid((kPvRow + kPvThreads - 1) / kPvThreads, (unsigned)L.B, 1);
    if (L.draw.seeds) {
        if (backward) hipLaunchKernelGGL((pv_frames_kernel<true, true>), grid, dim3(kPvThreads), 0, st, L);
        else hipLaunchKernelGGL((pv_frames_kernel<true, false>), grid, dim3(kPvThreads), 0, st, L);
    } else {
        if (backward) hipLaunchKernelGGL((pv_frames_kernel<false, true>), grid, dim3(kPvThreads), 0, st, L);
        else hipLaunchKernelGGL((pv_frames_kernel<false, false>), grid, dim3(kPvThreads), 0, st, L);
    }
}

void launch_pv_idle(const PvLaunch& L, const float* src, float* dst, hipStream_t st) {
    hipLaunchKernelGGL(pv_idle_kernel, dim3((unsigned)L.draw.pstride, (unsigned)L.B, 1), dim3(256), 0, st, L, src, dst);
}

}  // namespace aware
