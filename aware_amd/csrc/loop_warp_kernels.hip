// Time warp (EXTENSION, parity unpinned: the reference has neither the attack nor a chain inside its loop): the clip played at
// a speed that moves inside it -- wow and flutter, a drifting sample clock, a deliberate desynchronisation.  The rate is
// piecewise linear in time between drawn breakpoints P = 2^e samples apart, and every read position is exact in 64-bit integers.
// DESIGN.md section 35; the host twin is aware_amd/embedding/loop_attacks.py::warp_positions / time_warp / apply_chain.
//
//   r = philox4x32_10((0, s, 1 + j, 1), (seed_b, 0x5EED)),  on = (r0 + 0.5) / 2^32 < prob,
//   e = e_lo + ((r2 * (e_hi - e_lo + 1)) >> 32),  P = 2^e,  ph = (r1 * P) >> 32
//   w_k = philox4x32_10((k / 4, s, 20 + j, 0), (seed_b, 0x5EED))[k % 4],  m_k = -D + ((w_k * (2 D + 1)) >> 32),  R_k = 65536 + m_k
//   A(0) = 0,  A(k + 1) = A(k) + P R_k + (((R_{k+1} - R_k) P) >> 1)                    (signed 64-bit, arithmetic shifts)
//   Pos(u) = A(k) + t R_k + (((R_{k+1} - R_k) t t) >> (e + 1)),  k = u >> e,  t = u & (P - 1)
//   p_i = Pos(i + ph) - Pos(ph),  i0 = p_i >> 16,  f = (p_i & 0xFFFF) / 65536
//   forward   z[i] = the Catmull-Rom tap of speed_interp.hpp at (i0, f), x zero outside [0, n);  0 where p_i > (n - 1) << 16
//   adjoint   gx[j] = sum over ascending i of w_{j - i0(i)}(f_i) gz[i]
//
// Pos is continuous at the breakpoints (t = P gives A(k + 1)) and strictly increasing: every rate is at least 58983 / 65536, and
// a step of Pos is at least min(R_k, R_{k+1}) - 1.
//
// warp_table_kernel (forward pass only): one workgroup per clip writes R_k and A(k) of the clip's breakpoints.  256 segments at a
// time, their lengths P R_k + (((R_{k+1} - R_k) P) >> 1) are scanned inside each wave and across the four through LDS, and a
// carry goes from chunk to chunk.  Integer sums are exact in any order, so a cumulative sum on the host gives the same bits.
// The backward pass reads the table; it does not draw again.
//
// warp_kernel: one kernel for both directions and both layouts; every thread owns four consecutive outputs.  Forward, it finds
// its segment and the offset inside it with a shift and a mask, steps them along and takes the speed change's taps.  Adjoint, it
// finds the first input whose position reaches (j0 - 2) << 16 -- a bisection over A(k), then one over t inside the segment,
// both in integers with a fixed number of steps -- and walks the at most eight inputs that can reach its four outputs in
// ascending order: seven units of position at a step of at least 58982 / 65536.  No atomics, no LDS, no scratch.  An entry that
// does not fire copies the clip.  Every index into the table is clamped to it, and every position read lies inside the clip.
#include "loop_stage.hpp"
#include "speed_interp.hpp"

namespace aware {

namespace {

constexpr int kWarpThreads = 256;
constexpr unsigned kWarpWord = 20u;       // third Philox counter word of entry j's rates is 20 + j

// one clip's table: breakpoints 0 .. K - 1, so segments 0 .. K - 2
struct WarpTable {
    const int* R; const long long* A;
    int K, e;
    long long P;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the position t samples into a segment that starts at A with the rate R0 and ends with R1
__device__ __forceinline__ long long warp_pos_in(long long A, int R0, int R1, int e, long long t) {
    return A + t * (long long)R0 + (((long long)(R1 - R0) * t * t) >> (e + 1));
}
// the segment of u and the offset inside it; behind the table's last segment the position stays at that segment's end
__device__ __forceinline__ void warp_locate(const WarpTable& w, long long u, int& k, long long& t) {
    k = (int)min(u >> w.e, (long long)(w.K - 2));
    t = min(u - ((long long)k << w.e), w.P);
}
__device__ __forceinline__ long long warp_pos(const WarpTable& w, long long u) {
    int k;
    long long t;
    warp_locate(w, u, k, t);
    return warp_pos_in(w.A[k], w.R[k], w.R[k + 1], w.e, t);
}

// a walk along consecutive u: the segment's three table values, reloaded where the walk crosses a breakpoint
struct WarpWalk {
    int k, R0, R1;
    long long t, A;
};
__device__ __forceinline__ void warp_walk_start(const WarpTable& w, long long u, WarpWalk& s) {
    warp_locate(w, u, s.k, s.t);
    s.R0 = w.R[s.k]; s.R1 = w.R[s.k + 1]; s.A = w.A[s.k];
}
__device__ __forceinline__ void warp_walk_step(const WarpTable& w, WarpWalk& s) {
    if (++s.t < w.P) return;
    if (s.k < w.K - 2) {
        ++s.k; s.t = 0;
        s.R0 = s.R1; s.R1 = w.R[s.k + 1]; s.A = w.A[s.k];
    } else {
        s.t = w.P;
    }
}

// The transposed resampling in gather form: g[0 .. 3] = gx[j0 .. j0 + 3] from gz[0 .. n); pos0 = Pos(ph)
__device__ __forceinline__ void warp_adjoint4(const float* __restrict__ gz, int n, const WarpTable& w, int ph, long long pos0, int j0,
                                              float g[4]) {
    g[0] = g[1] = g[2] = g[3] = 0.f;
    const long long lo = ((long long)j0 - 2) << 16, plim = (long long)(n - 1) << 16;
    long long u = ph;
    if (lo > 0) {
        // the first u with Pos(u) >= T.  The last segment that starts at or below T: A(0) = 0 <= T
        const long long T = lo + pos0;
        int kl = 0, kh = w.K - 2;
#pragma unroll 1
        for (int s = 0; s < 24 && kl < kh; ++s) {              // K - 1 <= 2^22 + 1 segments: 23 halvings at the most
            const int mid = (kl + kh + 1) >> 1;
            if (w.A[mid] <= T) kl = mid; else kh = mid - 1;
        }
        // the least t in [0, P] inside it whose position reaches T (P itself: the start of the next segment)
        const int R0 = w.R[kl], R1 = w.R[kl + 1];
        const long long A = w.A[kl];
        long long tl = 0, th = w.P;
#pragma unroll 1
        for (int s = 0; s < 21 && tl < th; ++s) {              // P <= 2^20: 21 halvings at the most
            const long long mid = (tl + th) >> 1;
            if (warp_pos_in(A, R0, R1, w.e, mid) >= T) th = mid; else tl = mid + 1;
        }
        u = max(((long long)kl << w.e) + tl, (long long)ph);
    }
    WarpWalk s;
    warp_walk_start(w, u, s);
    long long i = u - ph;
#pragma unroll 1
    for (int c = 0; c < 8 && i < n; ++c, ++i) {
        const long long p = warp_pos_in(s.A, s.R0, s.R1, w.e, s.t) - pos0;
        const int i0 = (int)(p >> 16);
        if (p > plim || i0 > j0 + 4) break;
        const SpeedWeights sw = speed_weights_at(p);
        const float v = gz[i];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int d = j0 + q - i0;
            const float wt = d == -1 ? sw.wm1 : (d == 0 ? sw.w0 : (d == 1 ? sw.w1 : sw.w2));
            if (d >= -1 && d <= 2) g[q] = fmaf(wt, v, g[q]);
        }
        warp_walk_step(w, s);
    }
}

// rate k of clip b: drawn inside the loop, given (and clamped) stand-alone
template <bool LOOP>
__device__ __forceinline__ int warp_rate(const WarpLaunch& a, int b, int k, unsigned seed, unsigned step) {
    if (LOOP) {
        unsigned r[4];
        philox4x32_10((unsigned)k >> 2, step, kWarpWord + (unsigned)a.draw.entry, 0u, seed, 0x5EEDu, r);
        const unsigned wk = (k & 3) == 0 ? r[0] : ((k & 3) == 1 ? r[1] : ((k & 3) == 2 ? r[2] : r[3]));
        return 65536 - a.depth + loop_below(wk, 2 * a.depth + 1);
    }
    return 65536 + clampi(a.rates[(size_t)b * a.stride + min(k, a.stride - 1)], -kWarpMaxDepth, kWarpMaxDepth);
}

template <bool LOOP>
__global__ __launch_bounds__(kWarpThreads) void warp_table_kernel(WarpLaunch a) {
    const int b = blockIdx.x;
    int n, e;
    unsigned seed = 0u, step = 0u;
    if (LOOP) {      // every condition is uniform across the workgroup
        if (loop_gate_skips(a.draw.gate, b)) return;
        n = kHop * (a.draw.frame_off[b + 1] - a.draw.frame_off[b] - 1);
        unsigned r[4];
        if (!loop_entry_draw(a.draw, b, r)) return;           // the stage kernel copies the clip and reads no table
        e = loop_uniform(r[2], a.e_lo, a.e_hi);
        seed = a.draw.seeds[b]; step = (unsigned)(*a.draw.step - a.draw.step_back);
    } else {
        n = a.len[b];
        if (n < 1) return;
        e = clampi(a.e[b], kWarpMinExp, kWarpMaxExp);
    }
    const int K = min(warp_breakpoints(n, e), a.stride);
    int* R = a.table_r + (size_t)b * a.stride;
    long long* A = a.table_a + (size_t)b * a.stride;
    const long long P = 1ll << e;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ long long s_tot[kWarpThreads / 64];
    long long carry = 0;
    for (int k0 = 0; k0 < K; k0 += kWarpThreads) {
        const int k = k0 + (int)threadIdx.x;
        int r0 = 0;
        long long inc = 0;
        if (k < K) {
            r0 = warp_rate<LOOP>(a, b, k, seed, step);
            const int r1 = warp_rate<LOOP>(a, b, k + 1, seed, step);
            inc = P * (long long)r0 + (((long long)(r1 - r0) * P) >> 1);
        }
        long long v = inc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long up = __shfl_up(v, o);
            if (lane >= o) v += up;
        }
        if (lane == 63) s_tot[wave] = v;
        __syncthreads();
        long long base = carry, total = 0;
#pragma unroll
        for (int wv = 0; wv < kWarpThreads / 64; ++wv) {
            if (wv < wave) base += s_tot[wv];
            total += s_tot[wv];
        }
        if (k < K) { R[k] = r0; A[k] = base + v - inc; }
        carry += total;
        __syncthreads();
    }
}

template <bool LOOP>
__global__ __launch_bounds__(kWarpThreads) void warp_kernel(WarpLaunch a) {
    const int b = blockIdx.y;
    const float* x;
    float* y;
    int n, q0, q1, ph;      // the clip's length, this workgroup's groups of four outputs [q0, q1), the phase
    bool on;
    WarpTable w;
    if (LOOP) {
        LoopStage s;
        if (!loop_stage_enter(a.draw, b, s)) return;
        x = a.in + s.so; y = a.out + s.so;
        n = s.n;
        q0 = s.jb0 * (kHop / 4); q1 = s.jb1 * (kHop / 4);
        on = s.on;
        w.e = loop_uniform(s.r[2], a.e_lo, a.e_hi);
        ph = loop_below(s.r[1], 1 << w.e);
    } else {
        n = a.len[b];
        if (n < 1) return;
        x = a.in + a.off[b]; y = a.out + a.off[b];
        q0 = blockIdx.x * kWarpThreads; q1 = q0 + kWarpThreads;
        on = true;
        w.e = clampi(a.e[b], kWarpMinExp, kWarpMaxExp);
        ph = clampi(a.ph[b], 0, (1 << w.e) - 1);
    }
    q1 = min(q1, (n + 3) / 4);
    w.P = 1ll << w.e;
    w.K = min(warp_breakpoints(n, w.e), a.stride);
    w.R = a.table_r + (size_t)b * a.stride;
    w.A = a.table_a + (size_t)b * a.stride;
    const long long pos0 = on ? warp_pos(w, ph) : 0;
    for (int q = q0 + threadIdx.x; q < q1; q += kWarpThreads) {
        const int i = 4 * q;
        float v[4];
        if (!on) {
            load4(x, n, i, v);
        } else if (a.adjoint) {
            warp_adjoint4(x, n, w, ph, pos0, i, v);
        } else {
            WarpWalk s;
            warp_walk_start(w, (long long)i + ph, s);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                v[c] = speed_tap_at(x, n, warp_pos_in(s.A, s.R0, s.R1, w.e, s.t) - pos0);
                warp_walk_step(w, s);
            }
        }
        store4<LOOP>(y, n, q, v);
    }
}

}  // namespace

void launch_time_warp(const WarpLaunch& L, hipStream_t st) {
    const bool loop = L.draw.frame_off != nullptr;
    if (!L.adjoint)
        hipLaunchKernelGGL(loop ? warp_table_kernel<true> : warp_table_kernel<false>, dim3((unsigned)L.B), dim3(kWarpThreads), 0, st, L);
    hipLaunchKernelGGL(loop ? warp_kernel<true> : warp_kernel<false>, stage_grid(L.draw, L.B, L.max_len, 4 * kWarpThreads),
                       dim3(kWarpThreads), 0, st, L);
}

}  // namespace aware
