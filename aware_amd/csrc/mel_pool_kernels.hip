// The detector's mel stage for an initial pool other than (2, 2): InstanceNorm over time ->
// GlobalStandardize per clip -> AvgPool1d(size, stride), size and stride 2..8 each, and the backward of the three, on the
// chunked family's data (detector_kernels.hip): xm [NF][Mp], per-chunk partials [B][pstride][2 Mp], stats, gstat, x0 [NP][Mp].
// The statistics do not depend on the pool -- frames the pool drops still count in them, as in the reference -- so
// mel_partial_stats_kernel is shared as it is and every scalar expression is mel_norm.hpp's.  Three kernels replace
// mel_apply_pool_kernel, mel_bwd_partial_kernel and mel_bwd_apply_kernel; each runs a workgroup per 32-frame chunk and clip.
//
// A clip of T frames has L_0 = pool_rows(T, size, stride) pooled rows (conv_taps.hpp), L_0 <= floor(T / 2), in the rows the
// batch allocates for floor(T / 2).  Forward: a chunk writes the rows whose window *starts* in it and reads across its end
// where the window does.  Backward, in gather form: frame t collects the rows tp with tp stride <= t < tp stride + size, which
// are tp = pool_rows(t, size, stride) .. min(L_0 - 1, floor(t / stride)) -- at most ceil(size / stride) of them, none on a
// dropped tail frame or in a gap (size < stride) -- in ascending order.  No atomics: a run repeats bit for bit.
//
// Shape, as in the family: thread = channel (loads and stores contiguous along the channel axis), two row groups, fixed trip
// counts, loads first from clamped indices, stores masked.  The loops over the window (size) and over the rows of a frame
// (ceil(size / stride)) have a run-time, wave-uniform trip count around the unrolled rows.  No clip reads another clip's rows.
#include "kernels.h"
#include "mel_chunked.hpp"

namespace aware {

static_assert(kMinPool >= 2, "a chunk of kMelChunk frames starts at most kMelChunk / 2 windows, and L_0 <= floor(T / 2)");

// forward: x0[r0 + tp][c] = (1 / size) sum over j ascending of u[tp stride + j][c] ginv for tp < L_0; padding channels and the
// rows L_0 .. the clip's 32-row boundary are zero (the plain GEMMs walk them); stats and gstat as mel_apply_pool_kernel
template <class Bank>
__global__ __launch_bounds__(256) void mel_pool_fwd_kernel(const float* __restrict__ xm, const int* __restrict__ frame_off,
                                                            const int* __restrict__ pool_off, const float* __restrict__ part,
                                                            int pstride, float* __restrict__ x0, float* __restrict__ stats,
                                                            float* __restrict__ gstat, int n_mels, int Mp, int size, int stride) {
    __shared__ float red[4];
    const Bank bk(n_mels, Mp);
    const int b = blockIdx.y;
    const int f0 = frame_off[b], T = frame_off[b + 1] - f0;
    const int t0 = blockIdx.x * kMelChunk;
    if (t0 >= T) return;
    const int nchunk = (T + kMelChunk - 1) / kMelChunk;
    const int c = threadIdx.x & 127, g = threadIdx.x >> 7;
    const float* pp = part + (size_t)b * pstride * 2 * bk.Mp;
    float mus[Bank::kGroups], rss[Bank::kGroups], M2s[Bank::kGroups];   // zero for padding channels
    float suu = 0.f;
#pragma unroll
    for (int j = 0; j < Bank::kGroups; ++j) {
        mus[j] = 0.f; rss[j] = 0.f; M2s[j] = 0.f;
        const int ch = 128 * j + c;
        if (j >= bk.ng || ch >= bk.n_mels) continue;
        float mu, M2;
        mel_merge(pp, nchunk, T, ch, bk.Mp, mu, M2);
        const float rs = mel_rs(M2, (float)T);
        mus[j] = mu; rss[j] = rs; M2s[j] = M2;
        if (g == 0) suu += mel_suu(rs, M2);
    }
    suu = block_sum(suu, red);
    const MelClip k = mel_clip(suu, (float)T, bk.n_mels);
    if (blockIdx.x == 0 && threadIdx.x == 0) mel_write_gstat(gstat, b, k, (float)T);
    const int L0 = pool_rows(T, size, stride);
    // the rows whose window starts in this chunk: at most kMelChunk / 2 of them (stride >= 2)
    const int tp0 = (t0 + stride - 1) / stride, tp1 = min(L0, (t0 + kMelChunk + stride - 1) / stride);
    // the zero rows L_0 .. the 32-row boundary, shared out as the (2, 2) pool shares its rows: kMelChunk / 2 per chunk, the
    // rest to the last chunk
    const int Tpad = (T / 2 + 31) & ~31;
    const bool last = (int)blockIdx.x == nchunk - 1;
    const int z0 = max(L0, (int)blockIdx.x * (kMelChunk / 2));
    const int z1 = last ? Tpad : min(Tpad, ((int)blockIdx.x + 1) * (kMelChunk / 2));
    const float inv = 1.0f / (float)size;
#pragma unroll
    for (int j = 0; j < Bank::kGroups; ++j) {
        const int ch = 128 * j + c;
        if (j >= bk.ng || ch >= bk.Mp) continue;
        const bool on = ch < bk.n_mels;
        if (blockIdx.x == 0 && g == 0) mel_write_stats(stats, (size_t)b * bk.Mp + ch, mus[j], rss[j], M2s[j]);
        const float* x = xm + (size_t)f0 * bk.Mp + ch;
        float* o = x0 + (size_t)pool_off[b] * bk.Mp + ch;
        const float mu = mus[j], rs = rss[j];
        if (tp0 < tp1) {
            constexpr int NI = kMelChunk / 4;
            float acc[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i) acc[i] = 0.f;
            for (int w = 0; w < size; ++w) {
                float xv[NI];
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    const int tc = min(tp0 + g + 2 * i, tp1 - 1);         // tc stride + w <= (L_0 - 1) stride + size - 1 < T
                    xv[i] = x[(size_t)(tc * stride + w) * bk.Mp];
                }
#pragma unroll
                for (int i = 0; i < NI; ++i) acc[i] += mel_u(xv[i], mu, rs) * k.ginv;
            }
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int tp = tp0 + g + 2 * i;
                if (tp < tp1) o[(size_t)tp * bk.Mp] = on ? acc[i] * inv : 0.f;   // padding channels stay zero
            }
        }
        for (int tp = z0 + g; tp < z1; tp += 2) o[(size_t)tp * bk.Mp] = 0.f;
    }
}

// dv = dL/d(standardised frame) of the NI frames t0g + 2 i of one channel: (1 / size) times the sum of dx0 over the rows whose
// window holds the frame, ascending.  d0: the clip's rows of dx0 at the channel; L0 >= 1; nterm = ceil(size / stride).
// Frames past the clip's end are computed from the last frame's rows and masked by the caller.
template <int NI>
__device__ __forceinline__ void mel_pool_dv(const float* __restrict__ d0, int Mp, int t0g, int T, int L0, int size, int stride,
                                            int nterm, float inv, float (&dv)[NI]) {
    int lo[NI], n[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int t = min(t0g + 2 * i, T - 1);
        lo[i] = pool_rows(t, size, stride);                               // the windows that ended before frame t
        n[i] = min(L0, t / stride + 1) - lo[i];                           // <= 0: a dropped tail frame, or a gap
        dv[i] = 0.f;
    }
    for (int m = 0; m < nterm; ++m) {
        float dd[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) dd[i] = d0[(size_t)min(lo[i] + m, L0 - 1) * Mp];
#pragma unroll
        for (int i = 0; i < NI; ++i) dv[i] += (m < n[i]) ? dd[i] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) dv[i] *= inv;
}

// backward partials: D1_c = sum_t dv, D2_c = sum_t dv * u over the chunk's frames
template <class Bank>
__global__ __launch_bounds__(256) void mel_pool_bwd_partial_kernel(const float* __restrict__ dx0, const float* __restrict__ xm,
                                                                    const int* __restrict__ frame_off,
                                                                    const int* __restrict__ pool_off,
                                                                    const float* __restrict__ stats, float* __restrict__ part,
                                                                    int pstride, int n_mels, int Mp, int size, int stride) {
    __shared__ float s1[2][128], s2[2][128];
    const Bank bk(n_mels, Mp);
    const int b = blockIdx.y;
    const int f0 = frame_off[b], T = frame_off[b + 1] - f0;
    const int t0 = blockIdx.x * kMelChunk;
    if (t0 >= T) return;
    const int L0 = pool_rows(T, size, stride);
    const int nterm = (size + stride - 1) / stride;
    const float inv = 1.0f / (float)size;
    const int c = threadIdx.x & 127, g = threadIdx.x >> 7;
    float* o = part + ((size_t)b * pstride + blockIdx.x) * 2 * bk.Mp;
    for (int j = 0; j < bk.ng; ++j) {
        const int ch = 128 * j + c;
        const bool on = ch < bk.n_mels;
        const int cc = min(ch, bk.n_mels - 1);
        const MelChan s = mel_read_stats(stats, (size_t)b * bk.Mp + cc);
        const float* x = xm + (size_t)f0 * bk.Mp + cc;
        const float* d0 = dx0 + (size_t)pool_off[b] * bk.Mp + cc;
        float a1 = 0.f, a2 = 0.f;
        if (L0 > 0) {
            constexpr int NI = kMelChunk / 2;
            float xv[NI], dv[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i) xv[i] = x[(size_t)min(t0 + g + 2 * i, T - 1) * bk.Mp];
            mel_pool_dv<NI>(d0, bk.Mp, t0 + g, T, L0, size, stride, nterm, inv, dv);
#pragma unroll
            for (int i = 0; i < NI; ++i)
                if (t0 + g + 2 * i < T) {
                    a1 += dv[i];
                    a2 += dv[i] * mel_u(xv[i], s.mu, s.rs);
                }
        }
        s1[g][c] = a1; s2[g][c] = a2;
        __syncthreads();
        if (g == 0 && ch < bk.Mp) {
            o[ch] = on ? s1[0][c] + s1[1][c] : 0.f;
            o[bk.Mp + ch] = on ? s2[0][c] + s2[1][c] : 0.f;
        }
        if (Bank::kGroups > 1) __syncthreads();
    }
}

// backward apply, in place on xm (xm <- dL/dxm; zero in the padding channels)
template <class Bank>
__global__ __launch_bounds__(256) void mel_pool_bwd_apply_kernel(const float* __restrict__ dx0, float* __restrict__ xm,
                                                                  const int* __restrict__ frame_off,
                                                                  const int* __restrict__ pool_off,
                                                                  const float* __restrict__ stats, const float* __restrict__ gstat,
                                                                  const float* __restrict__ part, int pstride, int n_mels, int Mp,
                                                                  int size, int stride) {
    __shared__ float red[4];
    const Bank bk(n_mels, Mp);
    const int b = blockIdx.y;
    const int f0 = frame_off[b], T = frame_off[b + 1] - f0;
    const int t0 = blockIdx.x * kMelChunk;
    if (t0 >= T) return;
    const int nchunk = (T + kMelChunk - 1) / kMelChunk;
    const int L0 = pool_rows(T, size, stride);
    const int nterm = (size + stride - 1) / stride;
    const float inv = 1.0f / (float)size;
    const int c = threadIdx.x & 127, g = threadIdx.x >> 7;
    const MelClip k = mel_read_gstat(gstat, b);
    const float* pp = part + (size_t)b * pstride * 2 * bk.Mp;
    float d1s[Bank::kGroups], d2s[Bank::kGroups];
    MelChan ss[Bank::kGroups];                      // read ahead of the sums, whose barriers would expose the loads
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int j = 0; j < Bank::kGroups; ++j) {
        d1s[j] = 0.f; d2s[j] = 0.f; ss[j] = MelChan{0.f, 0.f, 0.f};
        const int ch = 128 * j + c;
        if (j >= bk.ng || ch >= bk.n_mels) continue;
        ss[j] = mel_read_stats(stats, (size_t)b * bk.Mp + ch);
        float D1 = 0.f, D2 = 0.f;
        for (int i = 0; i < nchunk; ++i) { D1 += pp[(size_t)i * 2 * bk.Mp + ch]; D2 += pp[(size_t)i * 2 * bk.Mp + bk.Mp + ch]; }
        d1s[j] = D1; d2s[j] = D2;
        if (g == 0) { sa += D1; sb += D2; }
    }
    sa = block_sum(sa, red);
    sb = block_sum(sb, red);
    const MelClipGrad q = mel_clip_grad(sa, sb, k);
    const int t1 = min(T, t0 + kMelChunk);
#pragma unroll
    for (int j = 0; j < Bank::kGroups; ++j) {
        const int ch = 128 * j + c;
        if (j >= bk.ng || ch >= bk.Mp) continue;
        float* x = xm + (size_t)f0 * bk.Mp + ch;
        if (ch >= bk.n_mels) {
            for (int t = t0 + g; t < t1; t += 2) x[(size_t)t * bk.Mp] = 0.f;
            continue;
        }
        const MelChan s = ss[j];
        const MelChanGrad m = mel_chan_grad(d1s[j], d2s[j], (float)T, s.rs, s.M2, k, q);
        const float* d0 = dx0 + (size_t)pool_off[b] * bk.Mp + ch;
        constexpr int NI = kMelChunk / 2;
        float xv[NI], dv[NI];
        // (a frame past the clip's end is loaded from frame T - 1, which the other row group may be overwriting: that value is
        //  dead -- the store below is masked by t < t1 and nothing else reads it -- as in mel_bwd_apply_kernel)
#pragma unroll
        for (int i = 0; i < NI; ++i) xv[i] = x[(size_t)min(t0 + g + 2 * i, T - 1) * bk.Mp];
        if (L0 > 0) {
            mel_pool_dv<NI>(d0, bk.Mp, t0 + g, T, L0, size, stride, nterm, inv, dv);
        } else {
#pragma unroll
            for (int i = 0; i < NI; ++i) dv[i] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int t = t0 + g + 2 * i;
            if (t < t1) x[(size_t)t * bk.Mp] = mel_bwd_value(dv[i], mel_u(xv[i], s.mu, s.rs), s.rs, k.ginv, q, m);
        }
    }
}

template <class Bank>
static void mel_pool_fwd(const float* xm, const int* frame_off, const int* pool_off, float* x0, float* stats, float* gstat,
                         float* part, int pstride, dim3 grid, int n_mels, int Mp, int size, int stride, hipStream_t st) {
    hipLaunchKernelGGL(mel_pool_fwd_kernel<Bank>, grid, dim3(256), 0, st, xm, frame_off, pool_off, part, pstride, x0, stats, gstat,
                       n_mels, Mp, size, stride);
}
template <class Bank>
static void mel_pool_bwd(const float* dx0, float* xm, const int* frame_off, const int* pool_off, const float* stats,
                         const float* gstat, float* part, int pstride, dim3 grid, int n_mels, int Mp, int size, int stride,
                         hipStream_t st) {
    hipLaunchKernelGGL(mel_pool_bwd_partial_kernel<Bank>, grid, dim3(256), 0, st, dx0, xm, frame_off, pool_off, stats, part,
                       pstride, n_mels, Mp, size, stride);
    hipLaunchKernelGGL(mel_pool_bwd_apply_kernel<Bank>, grid, dim3(256), 0, st, dx0, xm, frame_off, pool_off, stats, gstat, part,
                       pstride, n_mels, Mp, size, stride);
}

// One launcher per direction (kernels.h).  Clips of every length take the chunked form; the 128-band instantiations for the
// card's bank, else the any-bank ones.
void launch_mel_pool_fwd(const float* xm, const int* frame_off, const int* pool_off, float* x0, float* stats, float* gstat,
                         float* part, int pstride, int B, int max_frames, int n_mels, int Mp, int size, int stride, hipStream_t st) {
    if (B < 1 || max_frames < 1) return;
    launch_mel_partial_stats(xm, frame_off, part, pstride, B, max_frames, n_mels, Mp, st);
    const dim3 grid((max_frames + kMelChunk - 1) / kMelChunk, B);
    if (n_mels == 128)
        mel_pool_fwd<MelBank128>(xm, frame_off, pool_off, x0, stats, gstat, part, pstride, grid, n_mels, Mp, size, stride, st);
    else
        mel_pool_fwd<MelBankAny>(xm, frame_off, pool_off, x0, stats, gstat, part, pstride, grid, n_mels, Mp, size, stride, st);
}
void launch_mel_pool_bwd(const float* dx0, float* xm, const int* frame_off, const int* pool_off, const float* stats,
                         const float* gstat, float* part, int pstride, int B, int max_frames, int n_mels, int Mp, int size,
                         int stride, hipStream_t st) {
    if (B < 1 || max_frames < 1) return;
    const dim3 grid((max_frames + kMelChunk - 1) / kMelChunk, B);
    if (n_mels == 128)
        mel_pool_bwd<MelBank128>(dx0, xm, frame_off, pool_off, stats, gstat, part, pstride, grid, n_mels, Mp, size, stride, st);
    else
        mel_pool_bwd<MelBankAny>(dx0, xm, frame_off, pool_off, stats, gstat, part, pstride, grid, n_mels, Mp, size, stride, st);
}

}  // namespace aware
