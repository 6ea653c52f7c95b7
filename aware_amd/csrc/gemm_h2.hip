// Clip-aligned detector GEMM on the f16 matrix pipe with f32-level arithmetic: two-term operand split, three products.
//
// gfx950 has no fast path for f32 operands (v_mfma_f32_32x32x2_f32 runs at 1/16 of the 16-bit MFMA rate).  gemm_x3.hip
// writes an f32 value as three bf16 terms and runs six partial products.  This file uses the other 16-bit format:
//     a * 2^s = h + l + e,   h = RN_f16(a 2^s),  l = RN_f16(a 2^s - h),  |e| <= 2^-23 |a 2^s|
// (binary16 has 11 significand bits.  An f32 value has 24: h keeps the top 11, the residual a 2^s - h is exact in f32 -- a
// signed integer of at most 13 bits in units of the value's last place -- and l keeps 11 bits and the sign of it: exact for
// three quarters of all values, off by ONE unit in the last place of the f32 value for the rest; measured rms 2^-24.5).  The product a*b
// is h_a h_b + h_a l_b + l_a h_b, the term l_a l_b (<= 2^-22 |ab|, rms 2^-24.6) is dropped: THREE v_mfma_f32_16x16x32_f16
// with f32 accumulation per k-step, half the matrix-pipe time of the six-product kernel, 2/3 of its LDS fragment traffic and
// weight bytes.  Each partial product is exact in f32 (22 significand bits).  Error of one product against the exact a*b:
// rms 2^-23.7, worst case 2^-21 (an f32 multiply: rms 2^-25.2, worst 2^-24) -- i.e. this pipe is NOT bit-for-bit f32
// arithmetic; what it keeps is the error LEVEL of an f32 dot product, which the f32 accumulation of K terms sets in both
// cases (measured below).  The exact alternative is gemm_x3.hip (conv_pipe 2).
//
// binary16's exponent range (normal down to 2^-14) makes the scale 2^s part of the format:
//   * weights: one power of two per output channel (row of Wt), chosen when the weights are packed so that the row's
//     largest magnitude lands in [2^13, 2^14); the inverse goes into the epilogue (exact).  A weight more than 2^15 below
//     its row maximum has a subnormal l: its absolute error is then <= 2^-39 of the row maximum -- far below the f32
//     rounding of the row's large entries, which is what bounds a dot product's error;
//   * activations / gradients: one power of two per CLIP, from the clip's max |x|, which every producing kernel leaves as
//     per-wave partial maxima (K/16 floats per clip: no atomics, nothing to reset) and the consumer reduces at start-up.
// Measured against fp64 beside the f32-input MFMA kernel in tests/test_gpu_kernels.py::test_gemm_clip_x3 (mode 2) on operands
// spanning 2^10 per row: at or below the f32 chain's error on every shape and epilogue.
//
// Tiling, staging, epilogues: as gemm_x3.hip (one 512-thread workgroup = all rows of one clip x 128 columns, a wave = all
// rows x 16 columns, A split on the fly into LDS in fragment order, B fragments straight from L2, InstanceNorm statistics
// in registers).  Reference semantics of the epilogues: detection/modules/conv1d.py:38-42.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "common.hpp"
#include "split_bf16.hpp"
#include "conv_block.hpp"

namespace aware {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------------
// packing (device): Wt [N][K] f32 row-major (row pitch ldw) -> [N/16][KS][plane 0..1][lane 0..63][8 f16] + inverse scales
// ---------------------------------------------------------------------------------------------------
static inline size_t h2_plane_bytes(int N, int K) { return (size_t)N * (size_t)(((K + 31) / 32) * 32) * 2 * sizeof(uint16_t); }
size_t h2_packed_bytes(int N, int K) { return h2_plane_bytes(N, K) + (size_t)N * sizeof(float); }
const float* h2_inv_scale(const void* packed, int N, int K) { return (const float*)((const char*)packed + h2_plane_bytes(N, K)); }

// power-of-two scale that brings a maximum magnitude `amax` into [2^13, 2^14), at most 2^126 (so that its inverse is a normal
// number): maxima below 2^-113 -- zero and subnormal f32 included -- get 2^126 and land below 2^13.  h + l then still holds
// every f32 value to within one unit in its last place, as above: a subnormal value is a multiple of 2^-149, i.e. of 2^-23
// after the scale, on or next to binary16's subnormal grid (2^-24).  (A scale of 1 for maxima below 2^-107 rounded such clips
// and weight rows to h = l = 0: the block put out its bias alone.)
__device__ __forceinline__ float h2_scale_for(float amax) {
    const int e = (int)((__float_as_uint(amax) >> 23) & 0xFFu);
    return __uint_as_float((unsigned)(267 - max(e, 14)) << 23);
}
__device__ __forceinline__ float h2_pow2_inverse(float s) {            // s is a power of two
    const unsigned e = (__float_as_uint(s) >> 23) & 0xFFu;
    return __uint_as_float((254u - e) << 23);
}

__global__ __launch_bounds__(64) void h2_row_scale_kernel(const float* __restrict__ Wt, int ldw, int K, float* __restrict__ binv) {
    const int n = blockIdx.x, lane = threadIdx.x;
    float m = 0.f;
    for (int k = lane; k < K; k += 64) m = fmaxf(m, fabsf(Wt[(size_t)n * ldw + k]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) binv[n] = h2_pow2_inverse(h2_scale_for(m));
}

__global__ __launch_bounds__(64) void h2_pack_kernel(const float* __restrict__ Wt, int ldw, int N, int K, int KS,
                                                      const float* __restrict__ binv, u32x4* __restrict__ out) {
    const int ks = blockIdx.x, nt = blockIdx.y, lane = threadIdx.x;
    const int n = nt * 16 + (lane & 15), k0 = ks * 32 + 8 * (lane >> 4);
    const float s = h2_pow2_inverse(binv[n]);
    unsigned h[4], l[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = k0 + 2 * j;
        const float x = k < K ? Wt[(size_t)n * ldw + k] * s : 0.f, y = k + 1 < K ? Wt[(size_t)n * ldw + k + 1] * s : 0.f;
        const f16x2 hh = {(_Float16)x, (_Float16)y};
        const f16x2 ll = {(_Float16)(x - (float)hh.x), (_Float16)(y - (float)hh.y)};
        h[j] = __builtin_bit_cast(unsigned, hh);
        l[j] = __builtin_bit_cast(unsigned, ll);
    }
    u32x4* o = out + ((size_t)(nt * KS + ks) * 2) * 64 + lane;
    o[0] = u32x4{h[0], h[1], h[2], h[3]};
    o[64] = u32x4{l[0], l[1], l[2], l[3]};
}

// Wt_dev: device [N][K] f32 (row pitch ldw), N % 16 == 0; out: device, h2_packed_bytes(N, K)
void launch_h2_pack(const float* Wt_dev, int ldw, int N, int K, void* out, hipStream_t st) {
    const int KS = (K + 31) / 32;
    float* binv = (float*)((char*)out + h2_plane_bytes(N, K));
    hipLaunchKernelGGL(h2_row_scale_kernel, dim3(N), dim3(64), 0, st, Wt_dev, ldw, K, binv);
    hipLaunchKernelGGL(h2_pack_kernel, dim3(KS, N / 16), dim3(64), 0, st, Wt_dev, ldw, N, K, KS, binv, (u32x4*)out);
}

// per-clip max |x| of a [clips * rows_per_clip][K] matrix into the partial layout the GEMM reads: entry 0 = the maximum,
// entries 1 .. K/16 - 1 = 0.  For operands whose producer does not leave the partials (tests, the small-batch mel kernels).
__global__ __launch_bounds__(256) void clip_amax_kernel(const float* __restrict__ A, int lda, int K, int rows_per_clip,
                                                         float* __restrict__ amax) {
    __shared__ float red[4];
    const int clip = blockIdx.x, tid = threadIdx.x;
    const int k4 = K >> 2;
    float m = 0.f;
    for (int i = tid; i < rows_per_clip * k4; i += 256) {
        const int r = i / k4, c = i % k4;
        const float4 v = *reinterpret_cast<const float4*>(A + (size_t)(clip * rows_per_clip + r) * lda + 4 * c);
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    const int np = K >> 4;
    if (tid < np) amax[(size_t)clip * 64 + tid] = tid == 0 ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : 0.f;
}
void launch_clip_amax(const float* A, int lda, int K, int rows_per_clip, int B, float* amax, hipStream_t st) {
    hipLaunchKernelGGL(clip_amax_kernel, dim3(B), dim3(256), 0, st, A, lda, K, rows_per_clip, amax);
}

// ---------------------------------------------------------------------------------------------------
// the K loop of one tile (8 waves, a wave = all 32 RG rows x 16 columns)
// ---------------------------------------------------------------------------------------------------
// (x, y) scaled by s -> packed f16 pairs of the two planes (v_pk_mul_f32, v_cvt_pk_f16_f32, 2 v_cvt_f32_f16, v_pk_fma_f32,
// v_cvt_pk_f16_f32: the residual is one exact fused multiply-subtract)
__device__ __forceinline__ void h2_split_pair(float x, float y, float s, unsigned& h, unsigned& l) {
    const float tx = x * s, ty = y * s;
    const f16x2 hh = {(_Float16)tx, (_Float16)ty};
    const f16x2 ll = {(_Float16)(tx - (float)hh.x), (_Float16)(ty - (float)hh.y)};
    h = __builtin_bit_cast(unsigned, hh);
    l = __builtin_bit_cast(unsigned, ll);
}

// acc[m][n] += (A[bm + 16 m .. +16)[0..K) * 2^sa) * (B 2^sb)^T for the wave's NT column tiles bn + 16 (NT wave + n) ..; the
// caller unscales.  `lds`: 2 * 2 * 2 * 2RG KiB of staging memory (two K tiles of 64, two K32 steps, two planes); every wave of
// the NW-wave workgroup calls this with the same arguments; the caller provides a barrier between two calls that reuse `lds`.
// NT = 1, NW = 8: a wave owns 16 columns, three MFMAs per A fragment read.  NT = 4, NW = 4 (the wide form): a wave owns 64
// columns, twelve MFMAs per A fragment read, and a workgroup of half the threads stages the rows for twice the columns.  Every
// accumulator sees the same products in the same order at any NT (l_a h_b, h_a l_b, h_a h_b per K32 step, ascending K): the
// forms are bit-identical.
template <int RG, int NT = 1, int NW = 8>
__device__ __forceinline__ void h2_tile_gemm(const float* __restrict__ A, int lda, const u32x4* __restrict__ Bpk, int K, int bm,
                                             int bn, unsigned char* lds, f32x4 (&acc)[2 * RG][NT], int row_limit, float ascale) {
    constexpr int MT = 2 * RG;            // 16-row tiles per clip
    constexpr int MH = RG;                // ... per half (the unit of the A-fragment schedule)
    constexpr int FRAG = 1024;            // one 16-row x 32-k f16 fragment image, bytes
    constexpr int PLANE = MT * FRAG;
    constexpr int KSS = 2 * PLANE;        // one K32 step
    constexpr int BUF = 2 * KSS;          // one K tile (BK = 64)
    // A staging: pass i covers rows RP i .. RP i + RP - 1 of the K tile; thread -> (row tid >> 4, 4 floats at k = 4 (tid & 15)):
    // one fully coalesced 16-byte load per lane (16 lanes = one 256-byte row segment) and one 8-byte LDS store per plane
    constexpr int RP = 4 * NW;            // rows per pass: 32 (8 waves) or 16 (4 waves)
    constexpr int NPASS = 32 * RG / RP;

    bm = __builtin_amdgcn_readfirstlane(bm);
    bn = __builtin_amdgcn_readfirstlane(bn);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, kg = lane >> 4;
    const int srow = tid >> 4, k4 = tid & 15, sc = k4 >> 1;      // sc: the 8-wide k chunk (one lane's share of a fragment)
    unsigned rb[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) rb[t] = (unsigned)(t * KSS + kg * 256 + ((r16 ^ (4 * t + kg)) * 16));

    const int KS2 = K >> 5;
    const int nkt = K >> 6;
    const u32x4* bp = Bpk + ((size_t)((bn >> 4) + wave * NT) * KS2) * 128;          // uniform; + lane per thread
    const float* ap = A + (size_t)bm * lda;                                          // uniform
    unsigned roff[NPASS];
#pragma unroll
    for (int i = 0; i < NPASS; ++i) roff[i] = (unsigned)(min(srow + RP * i, row_limit - 1) * lda + k4 * 4);
    // LDS slot of this thread's 4 k-values of row srow (+ RP i: RP / 16 fragment images further): the XOR of the row slot with
    // the k chunk keeps the 16 lanes of a row on 16 distinct 8-byte slots of a 128-byte bank row
    const unsigned woff = (unsigned)((sc >> 2) * KSS + (srow >> 4) * FRAG + (sc & 3) * 256 + (((srow & 15) ^ sc) * 16) + (k4 & 1) * 8);

#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    float4 ra[NPASS];
    auto gload_c = [&](int i, int kt) { ra[i] = *reinterpret_cast<const float4*>(ap + kt * 64 + roff[i]); };
    auto split_store_c = [&](int i, unsigned boff) {
        uint2 qh, ql;
        h2_split_pair(ra[i].x, ra[i].y, ascale, qh.x, ql.x);
        h2_split_pair(ra[i].z, ra[i].w, ascale, qh.y, ql.y);
        unsigned char* d = lds + boff + woff + i * (RP / 16) * FRAG;
        *reinterpret_cast<uint2*>(d) = qh;
        *reinterpret_cast<uint2*>(d + PLANE) = ql;
    };
    // B fragments one K32 step ahead (two steps ahead measured no different)
    u32x4 bq[2][2][NT];
    auto loadB = [&](int set, int ks2) {
        ks2 = ks2 < KS2 ? ks2 : KS2 - 1;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int p = 0; p < 2; ++p) bq[set][p][n] = (bp + (((size_t)n * KS2 + ks2) * 2 + p) * 64)[(unsigned)lane];
    };
    auto lds_barrier = [&]() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    // A fragments: the h plane is double-buffered (the next quarter's h fragments are requested a whole quarter -- 3 MH MFMAs
    // -- ahead), the l plane single-buffered and refilled right after its only product of the quarter (2 MH MFMAs ahead)
    f16x8 ah[2][MH], al[MH];
    auto read_h = [&](int set, unsigned off) {
#pragma unroll
        for (int m = 0; m < MH; ++m) ah[set][m] = *reinterpret_cast<const f16x8*>(lds + off + m * FRAG);
    };
    auto read_l = [&](unsigned off) {
#pragma unroll
        for (int m = 0; m < MH; ++m) al[m] = *reinterpret_cast<const f16x8*>(lds + off + PLANE + m * FRAG);
    };
    // (column tile outermost: consecutive MFMAs never share an accumulator)
#define H2_MFMA(a_, b_, hf_)                                                                                                   \
    _Pragma("unroll") for (int n = 0; n < NT; ++n)                                                                             \
    _Pragma("unroll") for (int m = 0; m < MH; ++m)                                                                             \
        acc[(hf_) * MH + m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16((a_)[m], __builtin_bit_cast(f16x8, (b_)[n]),           \
                                                                        acc[(hf_) * MH + m][n], 0, 0, 0)
#define H2_PIN(mask, n) __builtin_amdgcn_sched_group_barrier(mask, n, 0)

#pragma unroll
    for (int i = 0; i < NPASS; ++i) gload_c(i, 0);
    loadB(0, 0);
#pragma unroll
    for (int i = 0; i < NPASS; ++i) split_store_c(i, 0);
#pragma unroll
    for (int i = 0; i < NPASS; ++i) gload_c(i, nkt > 1 ? 1 : 0);
    lds_barrier();
    read_h(0, rb[0]);
    read_l(rb[0]);
    for (int kt = 0; kt < nkt; ++kt) {
        const unsigned cur = (kt & 1) * BUF, nxt = BUF - cur;
        const int ktn = kt + 2 < nkt ? kt + 2 : nkt - 1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {                 // quarter = (K32 step q>>1, row half q&1)
            const int t = q >> 1, hf = q & 1;
            if (hf == 0) loadB((t + 1) & 1, kt * 2 + t + 1);
#pragma unroll
            for (int i = q; i < NPASS; i += 4) {
                split_store_c(i, nxt);
                gload_c(i, ktn);
            }
            const unsigned noff = q < 3 ? cur + rb[(q + 1) >> 1] + ((q + 1) & 1) * MH * FRAG : nxt + rb[0];
            if (q < 3) { read_h((q + 1) & 1, noff); H2_PIN(0x100, MH); }
            H2_MFMA(al, bq[t][0], hf);                // l_a * h_b
            H2_PIN(0x008, MH * NT);
            if (q == 3) {                             // tile kt+1 is complete; every wave has finished its reads of tile kt
                lds_barrier();
                read_h(0, noff);
                H2_PIN(0x100, MH);
            }
            read_l(noff);
            H2_PIN(0x100, MH);
            // raised priority around the h_a cluster of a quarter: -1.3 % per iteration (alternating runs on one box); around the
            // l_a cluster too: no further change; a static priority for waves 4..7 instead: +0.8 %
            __builtin_amdgcn_s_setprio(1);
            H2_MFMA(ah[q & 1], bq[t][1], hf);         // h_a * l_b
            H2_MFMA(ah[q & 1], bq[t][0], hf);         // h_a * h_b
            H2_PIN(0x008, 2 * MH * NT);
            __builtin_amdgcn_s_setprio(0);
        }
    }
#undef H2_PIN
#undef H2_MFMA
}

// the f16x2 operand format of the shared conv block bodies (conv_block.hpp)
struct H2Ops {
    static constexpr bool kScaled = true;
    static constexpr int kWeightBytes = 4;        // two f16 terms
    static constexpr int kTerms = 2;
    template <int RG, int NT = 1, int NW = 8>
    __device__ static __forceinline__ void tile_gemm(const float* __restrict__ A, int lda, const u32x4* __restrict__ Bpk, int K,
                                                     int bm, int bn, unsigned char* lds, f32x4 (&acc)[2 * RG][NT], int row_limit,
                                                     float ascale) {
        h2_tile_gemm<RG, NT, NW>(A, lda, Bpk, K, bm, bn, lds, acc, row_limit, ascale);
    }
    __device__ static __forceinline__ float scale_for(float amax) { return h2_scale_for(amax); }
    __device__ static __forceinline__ float pow2_inverse(float s) { return h2_pow2_inverse(s); }
};

// the conv block / data-gradient kernel for uniform batches (epilogues as gemm_clip_x3_kernel, plus the per-clip scales).
// NT x NW = 1 x 8: 128-column slabs, 512 threads, <= 128 VGPRs for RG <= 3 (two workgroups per CU).  4 x 4 (the wide form,
// RG <= 3): 256-column slabs, 256 threads at two waves per SIMD (again two workgroups per CU).
// ROWS (wide form only): the row-major epilogue of conv_block_uniform, chosen by the launcher.
template <int RG, int EPI, int NT = 1, int NW = 8, bool ROWS = false>
__global__ __launch_bounds__(64 * NW, NT > 1 ? 2 : RG <= 3 ? 4 : 2) void gemm_clip_h2_kernel(
    const float* __restrict__ A, int lda, const u32x4* __restrict__ Bpk, const float* __restrict__ binv,
    const float* __restrict__ amax_in, float* __restrict__ amax_out, const float* __restrict__ bias, float* __restrict__ C, int ldc,
    int Tp, int N, int K, int tiles_n, int ntiles, float* __restrict__ rstd_io, const float* __restrict__ act,
    const u32x4* __restrict__ Lpk, float* __restrict__ zpart, int CL) {
    conv_block_uniform<H2Ops, RG, EPI, NT, NW, ROWS>(A, lda, Bpk, binv, amax_in, amax_out, bias, C, ldc, Tp, N, K, tiles_n, ntiles,
                                                     rstd_io, act, Lpk, zpart, CL, 0);
}

// Ragged batches (as gemm_ragged_x3_kernel): the clip's scale comes from amax_in as in the uniform kernel; the partial maxima
// of the output (per 16-column group, over all chunks) go to amax_out.
template <int EPI>
__global__ __launch_bounds__(512, 4) void gemm_ragged_h2_kernel(const float* __restrict__ A, int lda, const u32x4* __restrict__ Bpk,
                                                                const float* __restrict__ binv, const float* __restrict__ amax_in,
                                                                float* __restrict__ amax_out, const float* __restrict__ bias,
                                                                float* __restrict__ C, int ldc, const int* __restrict__ frame_off,
                                                                const int* __restrict__ pool_off, const int* __restrict__ order, int N,
                                                                int K, int tiles_n, int ntiles, float* __restrict__ rstd_io,
                                                                const float* __restrict__ act) {
    conv_block_ragged<H2Ops, EPI>(A, lda, Bpk, binv, amax_in, amax_out, bias, C, ldc, frame_off, pool_off, order, N, K, tiles_n,
                                  ntiles, rstd_io, act);
}

// epi: 1 forward, 2 backward (as launch_gemm_ragged_x3); amax_in / amax_out as launch_gemm_clip_h2
void launch_gemm_ragged_h2(const float* A, int lda, const void* Bpk, const float* amax_in, float* amax_out, const float* bias,
                           float* C, int ldc, int B, const int* frame_off, const int* pool_off, const int* order, int N, int K,
                           int epi, float* rstd_io, const float* act, hipStream_t st) {
    const int tn = N / 128;
    const float* binv = h2_inv_scale(Bpk, N, K);
    constexpr size_t kLds = ragged_lds_bytes<H2Ops>();
    if (epi == X3_FWD)
        hipLaunchKernelGGL((gemm_ragged_h2_kernel<X3_FWD>), dim3(tn * B), dim3(512), kLds, st, A, lda, (const u32x4*)Bpk, binv, amax_in,
                           amax_out, bias, C, ldc, frame_off, pool_off, order, N, K, tn, tn * B, rstd_io, act);
    else
        hipLaunchKernelGGL((gemm_ragged_h2_kernel<X3_BWD>), dim3(tn * B), dim3(512), kLds, st, A, lda, (const u32x4*)Bpk, binv, amax_in,
                           amax_out, bias, C, ldc, frame_off, pool_off, order, N, K, tn, tn * B, rstd_io, act);
}

// per-clip max |x| over the clip's pooled rows (ragged layout), into the partial layout: entry 0 = the maximum, 1 .. K/16-1 = 0
__global__ __launch_bounds__(256) void ragged_amax_kernel(const float* __restrict__ A, int lda, int K, const int* __restrict__ frame_off,
                                                           const int* __restrict__ pool_off, float* __restrict__ amax) {
    __shared__ float red[4];
    const int clip = blockIdx.x, tid = threadIdx.x;
    const int Tp = (frame_off[clip + 1] - frame_off[clip]) / 2, row0 = pool_off[clip];
    const int k4 = K >> 2;
    float m = 0.f;
    for (int i = tid; i < Tp * k4; i += 256) {
        const int r = i / k4, c = i % k4;
        const float4 v = *reinterpret_cast<const float4*>(A + (size_t)(row0 + r) * lda + 4 * c);
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    const int np = K >> 4;
    if (tid < np) amax[(size_t)clip * 64 + tid] = tid == 0 ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : 0.f;
}
void launch_ragged_amax(const float* A, int lda, int K, const int* frame_off, const int* pool_off, int B, float* amax, hipStream_t st) {
    hipLaunchKernelGGL(ragged_amax_kernel, dim3(B), dim3(256), 0, st, A, lda, K, frame_off, pool_off, amax);
}

bool gemm_clip_h2_supported(int nwm, int N, int K, int lda) {
    return nwm >= 1 && nwm <= 4 && N % 128 == 0 && K % 64 == 0 && K <= 1024 && lda % 4 == 0;
}
// the wide form (tile 2 of launch_gemm_clip_h2): clips of at most three 32-row groups (four do not fit the register file: 256
// VGPRs and 46 spilled in the K loop alone), whole 256-column slabs
bool gemm_clip_h2_wide_supported(int nwm, int N, int K, int lda) {
    return gemm_clip_h2_supported(nwm, N, K, lda) && nwm <= 3 && N % kH2WideTile == 0;
}

// Wave arrangement.  Two forms, bit-identical (tests/test_gpu_conv_wide_tile.py), chosen once per plan (capi.hip, det_plan):
//   tile 1   8 waves x 1 column tile (128-column slabs, <= 128 VGPRs, two workgroups per CU).  Per wave and K tile at RG = 3:
//            36 MFMA, 24 ds_read_b128, 3 LDS stores, 7 global loads, 51 VALU; the A rows of a clip are loaded, split and
//            staged by N / 128 workgroups.
//   tile 2   4 waves x 4 column tiles (256-column slabs, the register file spent on 24 accumulators per wave, two waves per
//            SIMD, two workgroups per CU; RG <= 3).  Per wave and K tile: 144 MFMA, the same 24 ds_read_b128 (twelve MFMAs per
//            fragment instead of three), 12 LDS stores, 22 global loads; the A work of a clip is done by N / 256
//            workgroups.
// Measured alternatives to tile 1 that kept 16 columns per wave or three to four waves per SIMD, on the five launches of an
// iteration at B = 256 (kernel trace of the launches alone, us): 8 x 1 543; 16 x 1 (256-column slabs, one 1024-thread
// workgroup per CU: half the A staging per MFMA) 510 -- but no difference inside the embed loop (1.025 vs 1.026 ms per iteration,
// alternating runs on one box); 8 x 2 (two tiles per wave, 150 VGPRs) 548; the same GEMM on v_mfma_f32_32x32x16_f16 (a wave =
// all rows x 32 columns: half the MFMA issues, LDS fragment reads and staging per multiply-add, at the 128-VGPR limit) 565;
// B fragments two K32 steps ahead instead of one: no change; the split arithmetic of a quarter spread behind its MFMAs (two
// vector instructions per MFMA, sched_group_barrier) instead of ahead of them: +3 % (the scheduler then exposes the fragment
// reads).  DESIGN.md section 4 has the counters behind this and the measurements of tile 2.

// Bpk: launch_h2_pack image of Wt [N][K]; amax_in: [B][64] partial maxima of A's clips (K/16 valid per clip); amax_out: the
// same for C ([B][64], N/16 written per clip) or null; lastpk / zpart / CL as launch_gemm_clip_x3 (gemm_x3.hip's pack, N / 128
// partial slabs at either tile).  tile: 1 or 2 (2 only where gemm_clip_h2_wide_supported).
// The epilogues of the wide form that take the row-major path where the buffers allow it (bit X3_*; conv_block.hpp, ROWS).
// A build may narrow the set to hold single epilogues against their accumulator-layout form.
#ifndef AWARE_H2_ROW_EPILOGUES
#define AWARE_H2_ROW_EPILOGUES ((1 << X3_PLAIN) | (1 << X3_FWD) | (1 << X3_BWD) | (1 << X3_FWD_LAST))
#endif
constexpr int kH2RowEpilogues = AWARE_H2_ROW_EPILOGUES;

// The form a launch takes: 1 = 128-column slabs, 2 = wide with the accumulator-layout epilogue, 3 = wide with the row-major
// epilogue, whose 16-byte accesses need ldc % 4 == 0 and 16-byte aligned C and act (last: the forward epilogue with lastpk / zpart).
int gemm_clip_h2_form(int tile, int nwm, int epi, bool last, const float* C, int ldc, const float* act) {
    if (tile != 2 || nwm > 3) return 1;
    if (epi == X3_FWD && last) epi = X3_FWD_LAST;
    const bool aligned = (ldc & 3) == 0 && ((uintptr_t)C & 15) == 0 && (epi != X3_BWD || ((uintptr_t)act & 15) == 0);
    return aligned && ((kH2RowEpilogues >> epi) & 1) ? 3 : 2;
}

void launch_gemm_clip_h2(const float* A, int lda, const void* Bpk, const float* amax_in, float* amax_out, const float* bias,
                         float* C, int ldc, int B, int nwm, int Tp, int N, int K, int epi, float* rstd_io, const float* act,
                         hipStream_t st, const void* lastpk, float* zpart, int CL, int tile) {
    const float* binv = h2_inv_scale(Bpk, N, K);
    const int form = gemm_clip_h2_form(tile, nwm, epi, lastpk && zpart, C, ldc, act);
    if (epi == X3_FWD && lastpk && zpart) epi = X3_FWD_LAST;
    const bool wide = form >= 2, rows = form == 3;
    const int tn = N / (wide ? kH2WideTile : 128);
#define HK(M_, E_, NT_, NW_, R_) hipLaunchKernelGGL((gemm_clip_h2_kernel<M_, E_, NT_, NW_, R_>), dim3(tn * B), dim3(64 * NW_), 0, st, \
                                                    A, lda, (const u32x4*)Bpk, binv, amax_in, amax_out, bias, C, ldc, Tp, N, K, tn,    \
                                                    tn * B, rstd_io, act, (const u32x4*)lastpk, zpart, CL)
#define HW(M_, E_) if (rows) HK(M_, E_, 4, 4, true); else HK(M_, E_, 4, 4, false)
#define HM(E_)                                                                                                                 \
    if (wide) switch (nwm) { case 1: HW(1, E_); break; case 2: HW(2, E_); break; default: HW(3, E_); break; }                    \
    else switch (nwm) { case 1: HK(1, E_, 1, 8, false); break; case 2: HK(2, E_, 1, 8, false); break;                            \
                        case 3: HK(3, E_, 1, 8, false); break; default: HK(4, E_, 1, 8, false); break; }
    if (epi == X3_FWD) { HM(X3_FWD) } else if (epi == X3_BWD) { HM(X3_BWD) } else if (epi == X3_FWD_LAST) { HM(X3_FWD_LAST) }
    else { HM(X3_PLAIN) }
#undef HM
#undef HW
#undef HK
}

}  // namespace aware
