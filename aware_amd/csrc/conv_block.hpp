// The conv block / data-gradient kernel bodies shared by gemm_x3.hip (three bf16 terms, six products) and gemm_h2.hip (two
// f16 terms with per-clip / per-row power-of-two scales, three products).  The two formats differ only in their K loops;
// everything around the K loop lives here once: the block -> (clip, slab) walk, the PLAIN / FWD / BWD / FWD_LAST epilogues of
// the uniform kernel, and the chunk walk with the one- and two-pass InstanceNorm of the ragged kernel.
//
// An operand-format policy P provides:
//   kScaled        false (x3): the products are the values.  true (h2): the clip's scale comes from the producer's partial
//                  maxima (amax_in), the epilogue multiplies by 2^-sa and then by binv[col] (two exact steps: their product
//                  underflows for a tiny clip against a small weight row while the output is still a normal number), and the
//                  output's partial maxima go to amax_out for the next GEMM;
//   kWeightBytes   packed bytes per weight (the slab-group size of the uniform walk);
//   kTerms         A terms staged in LDS (the staging buffer of one K tile is 2 kTerms MT KiB);
//   tile_gemm<RG>  the K loop: acc[m][0] = A[bm + 16 m ..][0..K) * B^T for the wave's 16 columns (scaled by ascale when kScaled);
//   tile_gemm<RG, NT, NW>  (formats with a wide form) the same for NT column tiles per wave in a workgroup of NW waves;
//   scale_for / pow2_inverse (kScaled only).
// A workgroup is 8 waves x 128 columns, a wave owning every row of its 16 columns -- or, in the wide form of the uniform f16x2
// kernel, 4 waves x 256 columns, a wave owning every row of 64.
// Reference semantics of the epilogues: detection/modules/conv1d.py:38-42 (conv -> InstanceNorm1d -> LeakyReLU) and its autograd.
#pragma once
#include <hip/hip_runtime.h>
#include "split_bf16.hpp"
#include "conv_epilogue_rows.hpp"

namespace aware {

constexpr int kConvFrag = 1024;        // one 16-row x 32-k 16-bit fragment image, bytes

// staging memory of the uniform kernel: two K tiles; FWD_LAST re-lays one 128-column slab of the output tile as f32
// [32 RG][132] in the same memory, then parks 8 x RG x 3 partial tiles of 1 KiB there
template <class P, int RG, int EPI>
constexpr int conv_block_lds_bytes() {
    constexpr int stage = 2 * 2 * P::kTerms * 2 * RG * kConvFrag;
    constexpr int last = 32 * RG * 132 * 4 > 8 * RG * 3 * kConvFrag ? 32 * RG * 132 * 4 : 8 * RG * 3 * kConvFrag;
    return (EPI == X3_FWD_LAST && last > stage) ? last : stage;
}

// columns of a workgroup's tile: NW waves x NT column tiles of 16
constexpr int conv_tile_width(int NT, int NW) { return 16 * NT * NW; }

// Slab-group size of the uniform walk: the largest divisor of tiles_n whose packed weights (sg * width * K * weight_bytes)
// fit 3.2 MB of an XCD's 4 MB L2 (host and device; tests/test_conv_tile_rule_host.py restates it)
__host__ __device__ inline int conv_slab_group(int tiles_n, int width, int K, int weight_bytes) {
    int sg = (int)(3355443u / (unsigned)(width * K * weight_bytes));
    sg = sg < 1 ? 1 : (sg > tiles_n ? tiles_n : sg);
    while (tiles_n % sg) --sg;
    return sg;
}

// ---------------------------------------------------------------------------------------------------
// uniform batches: one workgroup = all 32 RG rows of one clip x one slab of 16 NT NW columns
// ---------------------------------------------------------------------------------------------------
// binv / amax_in / amax_out: kScaled only.  Mrows (x3, PLAIN only): rows of A and C that exist; the last row block may be
// partial (reads clamped, stores masked).  tiles_n = N / (16 NT NW).
// NT column tiles per wave, NW waves: 1 x 8 (128-column slabs) everywhere, and 4 x 4 (256-column slabs, the wide form of the
// f16 two-term kernel).  The epilogue walks a wave's column tiles one after the other with the arithmetic of the 1 x 8 form on
// each, so every output, statistic and partial maximum has the same bits at any NT.
// ROWS (wide form only; needs ldc % 4 == 0 and 16-byte aligned C and act, which the launcher checks): C leaves, and the data
// gradient's `act` arrives, in ROW-MAJOR order -- 16 bytes per lane, every wave instruction eight whole 128-byte row pieces --
// turned through a wave-private quarter of the staging memory (conv_epilogue_rows.hpp), instead of in the accumulator's
// layout (four 64-byte row pieces per instruction).  Only the path between register and memory differs: same bits.
template <class P, int RG, int EPI, int NT = 1, int NW = 8, bool ROWS = false>
__device__ __forceinline__ void conv_block_uniform(const float* __restrict__ A, int lda, const u32x4* __restrict__ Bpk,
                                                   const float* __restrict__ binv, const float* __restrict__ amax_in,
                                                   float* __restrict__ amax_out, const float* __restrict__ bias,
                                                   float* __restrict__ C, int ldc, int Tp, int N, int K, int tiles_n, int ntiles,
                                                   float* __restrict__ rstd_io, const float* __restrict__ act,
                                                   const u32x4* __restrict__ Lpk, float* __restrict__ zpart, int CL, int Mrows) {
    constexpr int MT = 2 * RG;            // 16-row tiles per clip
    constexpr int MH = RG;
    constexpr int FRAG = kConvFrag;
    constexpr int W = conv_tile_width(NT, NW);
    static_assert(NT == 1 || P::kScaled, "the row-major PLAIN epilogue of the unscaled format is written for one column tile");
    static_assert(W % 128 == 0 && (NW == 8 || NW == 4), "FWD_LAST works on whole 128-column slabs with 4 or 8 waves");
    static_assert(!ROWS || (NT == 4 && NW == 4 && P::kScaled), "the row-major epilogue is written for the wide form");
    __shared__ __attribute__((aligned(16))) unsigned char lds[conv_block_lds_bytes<P, RG, EPI>()];

    // Blocks b and b + 8 share an XCD (observed round-robin placement; speed only).  An XCD takes a contiguous range of clips and
    // walks it slab-group-major: `sg` column slabs at a time whose packed weights (sg * W * K * kWeightBytes) fit its 4 MB L2
    // together with the activation rows in flight, all clips of the range for that group, then the next group.  Clip-major
    // order streamed all 6.3 MB of a 1024 x 1024 bf16x3 layer through the L2 for every clip (PMC: 565 MB fetched per launch for
    // 206 MB of operands); this order fetches the weights once per XCD and the activation rows once per group.
    int id = blockIdx.x;
    int clip, slab;
    if ((ntiles & 7) == 0) {
        const int x = id & 7, j = id >> 3, R = ntiles >> 3;          // XCD, index inside its range, workgroups per XCD
        const int nclip = R / tiles_n;                                // clips per XCD (ntiles = clips * tiles_n, clips % 8 == 0 here
        if (nclip * tiles_n == R && nclip > 0) {                     //  whenever the batch size is a multiple of 8)
            const int sg = conv_slab_group(tiles_n, W, K, P::kWeightBytes);
            const int per_group = nclip * sg;
            const int grp = j / per_group, r = j % per_group;
            clip = x * nclip + r / sg;
            slab = grp * sg + r % sg;
        } else {
            id = x * R + j;
            clip = id / tiles_n;
            slab = id % tiles_n;
        }
    } else {
        clip = id / tiles_n;
        slab = id % tiles_n;
    }
    const int bm = clip * 32 * RG;
    const int bn = slab * W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    const int col0 = bn + wave * (16 * NT) + r16;      // this lane's column of the wave's first column tile

    float ascale = 1.f, ainv = 1.f;
    if constexpr (P::kScaled) {
        // the clip's scale from the producer's partial maxima (K/16 of them: one per wave of each of its workgroups)
        float am = lane < (K >> 4) ? amax_in[(size_t)clip * 64 + lane] : 0.f;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) am = fmaxf(am, __shfl_xor(am, o));
        ascale = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(P::scale_for(am))));
    }

    f32x4 acc[MT][NT];
    const int row_limit = (!P::kScaled && EPI == X3_PLAIN) ? min(32 * RG, Mrows - bm) : 32 * RG;
    if constexpr (NT == 1 && NW == 8) P::template tile_gemm<RG>(A, lda, Bpk, K, bm, bn, lds, acc, row_limit, ascale);
    else P::template tile_gemm<RG, NT, NW>(A, lda, Bpk, K, bm, bn, lds, acc, row_limit, ascale);

    // ---- epilogue: lane holds rows m*16 + 4*kg + e (e = 0..3) of columns col0 + 16 n ----
    if constexpr (P::kScaled) ainv = P::pow2_inverse(ascale);
    const float invT = 1.0f / (float)Tp;
    if constexpr (!P::kScaled && EPI == X3_PLAIN) {
        if ((ldc & 3) == 0) {
            // The tile leaves in ROW-MAJOR order (16 bytes per lane, half a wave = one 512-byte row segment), not in the
            // accumulator's layout (4 rows x 64 bytes per wave instruction, which streams at about half the rate: measured on
            // the read-out kernel, 3.0 vs 6 TB/s).  The staging LDS is free now; pitch 132 floats keeps both sides conflict-free.
            float (*T)[132] = reinterpret_cast<float (*)[132]>(lds);
            const float bv = bias ? bias[col0] : 0.f;
            __syncthreads();                                // every wave has left the K loop
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) T[16 * m + 4 * kg + e][16 * wave + r16] = acc[m][0][e] + bv;
            __syncthreads();
            const int c4 = (lane & 31) * 4, rr = 2 * wave + (lane >> 5);
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                const int row = rr + 16 * j;
                float4 o = *reinterpret_cast<const float4*>(&T[row][c4]);
                if (row >= Tp) o = make_float4(0.f, 0.f, 0.f, 0.f);
                if (bm + row < Mrows) *reinterpret_cast<float4*>(C + (size_t)(bm + row) * ldc + bn + c4) = o;
            }
            return;
        }
    }
    // (the 128-column form keeps the accumulator-layout stores: at four waves per SIMD, behind the K loop of a second resident
    //  workgroup, they are hidden -- the row-major form measured the same time on the three conv blocks.  The wide form has two
    //  waves per SIMD to hide them behind and takes the row-major path, ROWS.)
    // ROWS: the wave's region [32 RG][32] f32 of the staging memory, one half (two column tiles) of its tile at a time
    namespace er = epi_rows;
    constexpr int RJ = ROWS ? er::row_passes(RG) : 1;
    constexpr bool kTurn = ROWS && EPI != X3_FWD_LAST;          // (FWD_LAST stores from the slab it lays out below)
    float* const reg = reinterpret_cast<float*>(lds) + wave * er::region_floats(RG);
    // what orders a wave's own LDS traffic: its DS instructions execute in order, the compiler must not move them
    auto wave_sync = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    // half h of the wave's tile in global memory, row-major: pass j = rows 8 j .. 8 j + 7, eight lanes per 128-byte piece
    auto half_offset = [&](int h, int j) {
        return (size_t)(bm + er::rm_row(lane, j)) * ldc + (bn + wave * (16 * NT) + 32 * h + er::rm_col(lane));
    };
    // the data gradient's `act`: the fragment registers of the K loop are dead, so both halves are requested at once, ahead of
    // the barrier (no spill at RG = 3 beside the 96 accumulators: 251 VGPRs)
    f32x4 ar[2][RJ];
    auto load_act = [&](int h) {
#pragma unroll
        for (int j = 0; j < RJ; ++j) ar[h][j] = *reinterpret_cast<const f32x4*>(act + half_offset(h, j));
    };
    if constexpr (kTurn) {
        if constexpr (EPI == X3_BWD) {
            load_act(0);
            load_act(1);
        }
        __syncthreads();                                    // every wave has left the K loop: the staging memory is free
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
    if constexpr (kTurn && EPI == X3_BWD) {
        if ((n & 1) == 0) {
#pragma unroll
            for (int j = 0; j < RJ; ++j) *reinterpret_cast<f32x4*>(reg + er::act_write(lane, j)) = ar[n >> 1][j];
            wave_sync();
        }
    }
    const int col = col0 + 16 * n;
    float bcol = 1.f;
    if constexpr (P::kScaled) bcol = binv[col];
    float omax = 0.f;                                   // max |output| of this column tile, for the next GEMM's scale
    if (EPI == X3_PLAIN) {
        const float bv = bias ? bias[col] : 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m * 16 + 4 * kg + e;
                const float o = row < Tp ? fmaf(acc[m][n][e] * ainv, bcol, bv) : 0.f;
                omax = fmaxf(omax, fabsf(o));
                if constexpr (ROWS) acc[m][n][e] = o;
                else if (P::kScaled || bm + row < Mrows) C[(size_t)(bm + row) * ldc + col] = o;
            }
    } else if (EPI == X3_FWD || EPI == X3_FWD_LAST) {
        const float bv = bias ? bias[col] : 0.f;
        float s = 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m * 16 + 4 * kg + e;
                acc[m][n][e] = fmaf(acc[m][n][e] * ainv, bcol, bv);
                if (row < Tp) s += acc[m][n][e];
            }
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        const float mean = s * invT;
        // The rounding of the centred values is spelled out: the bf16x3 kernel centres on the rounded mean and sums rounded
        // squares, the f16x2 kernel centres with the mean fused in (x - s / T in one fma) and sums fused squares -- what
        // each kernel computed before the two shared this body (left to fp contraction, the choice follows the vectoriser).
        auto centre = [&](float x) {
            if constexpr (P::kScaled) return fmaf(-invT, s, x);
            else return x - mean;
        };
        float qq = 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m * 16 + 4 * kg + e;
                if (row < Tp) {
                    const float d = centre(acc[m][n][e]);
                    if constexpr (P::kScaled) qq = fmaf(d, d, qq);
                    else qq += d * d;
                }
            }
        qq += __shfl_xor(qq, 16);
        qq += __shfl_xor(qq, 32);
        const float rs = 1.0f / sqrtf(qq * invT + 1e-5f);      // biased variance, eps 1e-5 (InstanceNorm1d defaults)
        if (kg == 0) rstd_io[(size_t)clip * N + col] = rs;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m * 16 + 4 * kg + e;
                const float u = centre(acc[m][n][e]) * rs;
                const float o = row < Tp ? (u > 0.f ? u : 0.2f * u) : 0.f;
                acc[m][n][e] = o;
                omax = fmaxf(omax, fabsf(o));
                if constexpr (!ROWS) C[(size_t)(bm + row) * ldc + col] = o;
            }
    } else {
        // X3_BWD: acc = dL/dA of the previous block's output (read from `act`, post-activation);
        //         C = dL/dZ = rstd * (dU - mean_t dU - u * mean_t(dU*u)),  dU = acc * lrelu'(u)
        const float rs = rstd_io[(size_t)clip * N + col];
        float s1 = 0.f, s2 = 0.f;
        float u[MT][4];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m * 16 + 4 * kg + e;
                // unconditional load (padding rows exist and hold zeros): a branch here would serialise the loads
                float av;
                if constexpr (ROWS) av = reg[er::act_read(lane, m, n & 1, e)];
                else av = act[(size_t)(bm + row) * ldc + col];
                const bool valid = row < Tp;
                const float uv = valid ? (av > 0.f ? av : av * 5.0f) : 0.f;                 // invert LeakyReLU(0.2)
                const float du = valid ? acc[m][n][e] * ainv * bcol * (av > 0.f ? 1.f : 0.2f) : 0.f;
                acc[m][n][e] = du;
                u[m][e] = uv;
                s1 += du;
                s2 += du * uv;
            }
        s1 += __shfl_xor(s1, 16);
        s1 += __shfl_xor(s1, 32);
        s2 += __shfl_xor(s2, 16);
        s2 += __shfl_xor(s2, 32);
        const float m1 = s1 * invT, m2 = s2 * invT;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m * 16 + 4 * kg + e;
                const float o = row < Tp ? rs * (acc[m][n][e] - m1 - u[m][e] * m2) : 0.f;
                omax = fmaxf(omax, fabsf(o));
                if constexpr (ROWS) acc[m][n][e] = o;
                else C[(size_t)(bm + row) * ldc + col] = o;
            }
    }
    if constexpr (kTurn) {
        // the finished column tile (zeros in its padding rows) goes to the region -- in the data gradient onto the slots its
        // `act` values were just read from; after the second tile of a half the half leaves in whole rows
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int e = 0; e < 4; ++e) reg[er::c_write(lane, m, n & 1, e)] = acc[m][n][e];
        if (n & 1) {
            wave_sync();
#pragma unroll
            for (int j = 0; j < RJ; ++j)
                *reinterpret_cast<float4*>(C + half_offset(n >> 1, j)) = *reinterpret_cast<const float4*>(reg + er::c_read(lane, j));
            wave_sync();
        }
    }
    if constexpr (P::kScaled) {
        if (amax_out) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) omax = fmaxf(omax, __shfl_xor(omax, o));
            if (lane == 0) amax_out[(size_t)clip * 64 + (col >> 4)] = omax;
        }
    }
    }
    if (EPI == X3_FWD_LAST) {
        // acc[m][n][e] holds this block's output (zero in padding rows).  The next conv block is the skinny last one
        // (CL <= 48 channels): its K = this N is split over the 128-column slabs, so this workgroup contributes, per slab of its
        // tile, the partial z_part[slab] = out[:, slab] * Wlast[:, slab]^T, on the bf16 pipe with the exact three-way split
        // whatever the format of the K loop (Lpk: gemm_x3.hip's pack).  A slab of the output tile is re-laid as A fragments
        // (k = column) in LDS.  Work units of a slab: (K32 step t = 0..3 of its 128 columns) x (half mh of the row tiles), all
        // column tiles of the last conv each; eight waves take one unit each (t = w>>1, mh = w&1), four waves take both halves
        // of step t = w.  The four t-partials are then summed through LDS in the order t = 0..3 at any wave count.
        const int KS2L = N >> 5, ncl = (CL + 15) >> 4;
        constexpr int UH = 8 / NW;                        // row halves per wave
        constexpr int WS = 8 / NT;                        // waves whose columns make one 128-column slab
        const int tq = NW == 8 ? wave >> 1 : wave, mh0 = NW == 8 ? wave & 1 : 0;
        float* const T = reinterpret_cast<float*>(lds);
        constexpr int TP = 132;
#pragma unroll
        for (int sl = 0; sl < W / 128; ++sl) {
        const int slab128 = (bn >> 7) + sl;
        bf16x8 bl[3][3];
#pragma unroll
        for (int n = 0; n < 3; ++n)
            if (n < ncl) {
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    bl[n][p] = __builtin_bit_cast(bf16x8, Lpk[(((size_t)n * KS2L + 4 * slab128 + tq) * 3 + p) * 64 + lane]);
            }
        __syncthreads();                                  // every wave is done with the staging buffers / the slab before
        // the slab goes through LDS as f32 [row][column], row pitch 132 floats (conflict-free 4-byte stores from
        // the accumulator layout); each wave reads its A fragments back as 8 consecutive columns per lane and splits them
        if (wave / WS == sl) {
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        T[(16 * m + 4 * kg + e) * TP + 16 * ((wave % WS) * NT + n) + r16] = acc[m][n][e];
        }
        __syncthreads();
        if constexpr (ROWS) {
            // C leaves from the slab: half a wave = one 512-byte row segment, eight rows per pass of the four waves
            const int c4 = (lane & 31) * 4, rr = 2 * wave + (lane >> 5);
#pragma unroll
            for (int j = 0; j < 4 * RG; ++j) {
                const int row = rr + 8 * j;
                *reinterpret_cast<float4*>(C + (size_t)(bm + row) * ldc + bn + 128 * sl + c4) =
                    *reinterpret_cast<const float4*>(T + row * TP + c4);
            }
        }
        f32x4 zt[UH * MH][3];
#pragma unroll
        for (int mm = 0; mm < UH * MH; ++mm) {
#pragma unroll
            for (int n = 0; n < 3; ++n) zt[mm][n] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float* src = T + (16 * (mh0 * MH + mm) + r16) * TP + 32 * tq + 8 * kg;
            const float4 x0 = *reinterpret_cast<const float4*>(src), x1 = *reinterpret_cast<const float4*>(src + 4);
            uint4 q0, q1, q2;
            split_pair(x0.x, x0.y, q0.x, q1.x, q2.x);
            split_pair(x0.z, x0.w, q0.y, q1.y, q2.y);
            split_pair(x1.x, x1.y, q0.z, q1.z, q2.z);
            split_pair(x1.z, x1.w, q0.w, q1.w, q2.w);
            bf16x8 a[3];
            a[0] = __builtin_bit_cast(bf16x8, q0); a[1] = __builtin_bit_cast(bf16x8, q1); a[2] = __builtin_bit_cast(bf16x8, q2);
#pragma unroll
            for (int term = 0; term < 6; ++term) {
                const int pa = term == 0 ? 2 : (term == 1 || term == 3) ? 1 : 0;
                const int pb = term == 2 ? 2 : (term == 1 || term == 4) ? 1 : 0;
#pragma unroll
                for (int n = 0; n < 3; ++n)
                    if (n < ncl) zt[mm][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[pa], bl[n][pb], zt[mm][n], 0, 0, 0);
            }
        }
        __syncthreads();                                  // all fragment reads done: the buffer becomes the partial store
        // partial of (step tq, row tile rt) at slot tq * MT + rt (with eight waves: (wave * MH + mm), as rt = mh0 * MH + mm)
#pragma unroll
        for (int mm = 0; mm < UH * MH; ++mm)
#pragma unroll
            for (int n = 0; n < 3; ++n)
                *reinterpret_cast<f32x4*>(lds + (size_t)((tq * MT + mh0 * MH + mm) * 3 + n) * FRAG + lane * 16) = zt[mm][n];
        __syncthreads();
        for (int rt = wave; rt < MT; rt += NW) {          // this wave finishes row tile rt
            float* zp = zpart + (size_t)slab128 * ((size_t)(ntiles / tiles_n) * 32 * RG * CL) + (size_t)(bm + 16 * rt + 4 * kg) * CL;
#pragma unroll
            for (int n = 0; n < 3; ++n)
                if (n < ncl) {
                    f32x4 t = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        t += *reinterpret_cast<const f32x4*>(lds + (size_t)((q * MT + rt) * 3 + n) * FRAG + lane * 16);
                    if (16 * n + r16 < CL) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) zp[(size_t)e * CL + 16 * n + r16] = t[e];
                    }
                }
        }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Ragged batches: the same conv block (or data-gradient GEMM) for clips of ANY length in ONE launch.
// A workgroup owns one clip x 128 columns, as above, but takes the clip's rows from the batch tables (pool_off is
// 32-aligned per clip, Tp = frames / 2) and walks them in chunks of at most three 32-row groups (<= 128 VGPRs: two workgroups
// per CU at any clip length).  A clip that fits one chunk gets the same single-pass epilogue as the uniform kernel
// (bit-identical results).  A longer clip is done in two passes over its chunks:
//   pass 1  GEMM of the chunk, raw result to C, per-column statistics carried in registers across the chunks
//           (forward: count / mean / M2 merged with Chan's formula; backward: the two sums of the InstanceNorm backward);
//   pass 2  the workgroup re-reads its own raw tile (L2-resident, written by the same lanes) and applies the
//           normalisation + LeakyReLU (forward) or the InstanceNorm backward (backward) in place.
// No second launch, no inter-workgroup traffic, the per-(clip, channel) statistics never leave the registers.  When kScaled,
// the clip's scale comes from amax_in as in the uniform kernel and the partial maxima of the output (per 16-column group, over
// all chunks) go to amax_out.
// ---------------------------------------------------------------------------------------------------
constexpr int kRaggedRG = 3;           // largest chunk, in 32-row groups
extern __shared__ __attribute__((aligned(16))) unsigned char conv_dyn_lds[];    // the ragged kernel's staging memory

template <class P>
constexpr size_t ragged_lds_bytes() { return 2 * 2 * P::kTerms * (2 * kRaggedRG) * kConvFrag; }     // two K tiles of the tallest chunk

template <class T>
__device__ __forceinline__ T* uniform_ptr(T* p) {
    // a wave-uniform pointer to GLOBAL memory that arrived as a function argument: in VGPRs and in the generic address
    // space (flat loads count on vmcnt AND lgkmcnt, so every wait in the K loop became a full drain of both).  Back to an
    // SGPR pair, and through address space 1 so that the loads are global_load again.
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (T*)(__attribute__((address_space(1))) T*)(((unsigned long long)hi << 32) | lo);
}

// one chunk: rows [bm, bm + 32 RG) of which `rows` are valid.  SINGLE: the clip is this chunk.
// st0/st1/st2: forward (count, mean, M2) of the column; backward (unused, sum dU, sum dU*u) in-lane partial sums;
// ascale / ainv / bcol / omax (kScaled only): the clip's scale, the epilogue's two factors (2^-sa, binv[col]), the running
// max |stored value| of this lane's column (single-pass clips).
// (not inlined: each tile height keeps its own register allocation -- inlined side by side the two K loops cost the
// kernel 20-40 spilled VGPRs inside the loop)
template <class P, int RG, int EPI>
__device__ __attribute__((noinline)) void ragged_chunk(const bool SINGLE, const float* __restrict__ A, int lda,
                                                       const u32x4* __restrict__ Bpk, const float* __restrict__ bias,
                                                       float* __restrict__ C, int ldc, int N, int K, int bm, int rows,
                                                       int store_rows, int bn, float* __restrict__ rstd_clip,
                                                       const float* __restrict__ act, float ascale, float ainv, float bcol, float& st0,
                                                       float& st1, float& st2, float& omax) {
    unsigned char* lds = conv_dyn_lds;
    // the arguments of a non-inlined function arrive in VGPRs; all of these are wave-uniform and go back to SGPRs (the K
    // loop runs at the 128-VGPR limit: left in VGPRs they were spilled and reloaded inside it)
    A = uniform_ptr(A); Bpk = uniform_ptr(Bpk); bias = uniform_ptr(bias); C = uniform_ptr(C);
    rstd_clip = uniform_ptr(rstd_clip); act = uniform_ptr(act);
    lda = __builtin_amdgcn_readfirstlane(lda); ldc = __builtin_amdgcn_readfirstlane(ldc);
    N = __builtin_amdgcn_readfirstlane(N); K = __builtin_amdgcn_readfirstlane(K);
    bm = __builtin_amdgcn_readfirstlane(bm); bn = __builtin_amdgcn_readfirstlane(bn);
    rows = __builtin_amdgcn_readfirstlane(rows); store_rows = __builtin_amdgcn_readfirstlane(store_rows);
    // rows: valid rows of the chunk; store_rows (a multiple of 32, <= 32 RG): rows of the clip's allocation under this tile
    if constexpr (P::kScaled) ascale = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(ascale)));
    else { ainv = 1.f; bcol = 1.f; }
    constexpr int MT = 2 * RG;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    f32x4 acc[MT][1];
    P::template tile_gemm<RG>(A, lda, Bpk, K, bm, bn, lds, acc, store_rows, ascale);
    const int col = bn + wave * 16 + r16;
    const float invR = 1.0f / (float)rows;
    auto track = [&](float o) { if constexpr (P::kScaled) omax = fmaxf(omax, fabsf(o)); };
    if (EPI == X3_FWD) {
        const float bv = bias ? bias[col] : 0.f;
        float s = 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[m][0][e] = fmaf(acc[m][0][e] * ainv, bcol, bv);
                if (m * 16 + 4 * kg + e < rows) s += acc[m][0][e];
            }
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        const float mean = s * invR;
        float qq = 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (m * 16 + 4 * kg + e < rows) { const float d = acc[m][0][e] - mean; qq += d * d; }
        qq += __shfl_xor(qq, 16);
        qq += __shfl_xor(qq, 32);
        if (SINGLE) {
            const float rs = 1.0f / sqrtf(qq * invR + 1e-5f);      // biased variance, eps 1e-5 (InstanceNorm1d defaults)
            if (kg == 0) rstd_clip[col] = rs;
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int row = m * 16 + 4 * kg + e;
                    const float u = (acc[m][0][e] - mean) * rs;
                    if (row < store_rows) {           // (rows <= store_rows: the rows skipped store and track zeros)
                        const float o = row < rows ? (u > 0.f ? u : 0.2f * u) : 0.f;
                        track(o);
                        C[(size_t)(bm + row) * ldc + col] = o;
                    }
                }
        } else {
            // raw conv output now, statistics merged across the clip's chunks (Chan et al.)
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int row = m * 16 + 4 * kg + e;
                    if (row < store_rows) C[(size_t)(bm + row) * ldc + col] = row < rows ? acc[m][0][e] : 0.f;
                }
            const float nc = (float)rows, nt = st0 + nc, dl = mean - st1;
            st2 = st2 + qq + dl * dl * (st0 * nc / nt);
            st1 = st1 + dl * (nc / nt);
            st0 = nt;
        }
    } else {      // X3_BWD
        float s1 = 0.f, s2 = 0.f;
        float u[MT][4];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m * 16 + 4 * kg + e;
                const float av = act[(size_t)(bm + min(row, store_rows - 1)) * ldc + col];   // unconditional (clamped, masked below)
                const bool valid = row < rows;
                const float uv = valid ? (av > 0.f ? av : av * 5.0f) : 0.f;                 // invert LeakyReLU(0.2)
                const float du = valid ? acc[m][0][e] * ainv * bcol * (av > 0.f ? 1.f : 0.2f) : 0.f;
                acc[m][0][e] = du;
                u[m][e] = uv;
                s1 += du;
                s2 += du * uv;
            }
        if (SINGLE) {
            const float rs = rstd_clip[col];
            s1 += __shfl_xor(s1, 16);
            s1 += __shfl_xor(s1, 32);
            s2 += __shfl_xor(s2, 16);
            s2 += __shfl_xor(s2, 32);
            const float m1 = s1 * invR, m2 = s2 * invR;
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int row = m * 16 + 4 * kg + e;
                    const float o = row < rows ? rs * (acc[m][0][e] - m1 - u[m][e] * m2) : 0.f;
                    track(o);
                    if (row < store_rows) C[(size_t)(bm + row) * ldc + col] = o;
                }
        } else {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int row = m * 16 + 4 * kg + e;
                    if (row < store_rows) C[(size_t)(bm + row) * ldc + col] = acc[m][0][e];          // dU (zero in padding rows)
                }
            st1 += s1;
            st2 += s2;
        }
    }
}

// order: dispatch position -> clip (longest first) or null
template <class P, int EPI>
__device__ __forceinline__ void conv_block_ragged(const float* __restrict__ A, int lda, const u32x4* __restrict__ Bpk,
                                                  const float* __restrict__ binv, const float* __restrict__ amax_in,
                                                  float* __restrict__ amax_out, const float* __restrict__ bias,
                                                  float* __restrict__ C, int ldc, const int* __restrict__ frame_off,
                                                  const int* __restrict__ pool_off, const int* __restrict__ order, int N, int K,
                                                  int tiles_n, int ntiles, float* __restrict__ rstd_io,
                                                  const float* __restrict__ act) {
    // blocks b and b + 8 share an XCD (observed round-robin placement; speed only): the slabs of one clip stay on one XCD
    // (its rows are read once into that L2), and clips are dealt to the XCDs round-robin -- batches arrive sorted by
    // length, a contiguous range per XCD would give one XCD all the long clips
    int clip, slab;
    {
        const int id = blockIdx.x, nclips = ntiles / tiles_n;
        if ((nclips & 7) == 0) {
            const int j = id >> 3;
            clip = (j / tiles_n) * 8 + (id & 7);
            slab = j % tiles_n;
        } else {
            clip = id / tiles_n;
            slab = id % tiles_n;
        }
        if (order) clip = order[clip];
    }
    const int bn = slab * 128;
    const int Tp = (frame_off[clip + 1] - frame_off[clip]) / 2;
    const int row0 = pool_off[clip];
    if (Tp < 1) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    const int col = bn + wave * 16 + r16;
    float ascale = 1.f, ainv = 1.f, bcol = 1.f;
    if constexpr (P::kScaled) {
        float am = lane < (K >> 4) ? amax_in[(size_t)clip * 64 + lane] : 0.f;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) am = fmaxf(am, __shfl_xor(am, o));
        ascale = P::scale_for(am);
        ainv = P::pow2_inverse(ascale);
        bcol = binv[col];
    }
    const int G = (Tp + 31) >> 5;                                   // 32-row groups of the clip
    const int nchunk = (G + kRaggedRG - 1) / kRaggedRG;
    const int gbase = G / nchunk, grem = G % nchunk;                // balanced: the first `grem` chunks take one group more
    float* rstd_clip = rstd_io + (size_t)clip * N;
    float st0 = 0.f, st1 = 0.f, st2 = 0.f, omax = 0.f;
    const bool single = nchunk == 1;
    int g0 = 0;
    for (int c = 0; c < nchunk; ++c) {
        const int ng = gbase + (c < grem ? 1 : 0);
        const int bm = row0 + 32 * g0;
        const int rows = min(32 * ng, Tp - 32 * g0);
        if (c) __syncthreads();                                     // every wave is done with the previous chunk's staging memory
        // two tile heights only (a one-group chunk runs as a two-group tile whose second group is padding: the K-order of
        // every output element is the same at any tile height, so the results do not depend on the choice)
        if (ng <= 2) ragged_chunk<P, 2, EPI>(single, A, lda, Bpk, bias, C, ldc, N, K, bm, rows, 32 * ng, bn, rstd_clip, act, ascale, ainv, bcol, st0, st1, st2, omax);
        else ragged_chunk<P, 3, EPI>(single, A, lda, Bpk, bias, C, ldc, N, K, bm, rows, 32 * ng, bn, rstd_clip, act, ascale, ainv, bcol, st0, st1, st2, omax);
        g0 += ng;
    }
    if (single) {
        if constexpr (P::kScaled) {
            if (amax_out) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) omax = fmaxf(omax, __shfl_xor(omax, o));
                if (lane == 0) amax_out[(size_t)clip * 64 + (col >> 4)] = omax;
            }
        }
        return;
    }
    // ---- pass 2 over the raw tile this workgroup wrote: ROW-MAJOR (lane = 4 consecutive columns, half a wave = one 512-byte
    // row segment), the per-column statistics handed over through LDS.  In the accumulator's layout (the lane that wrote a
    // value reads it back: 4 rows x 64 bytes per wave instruction) this pass streamed at about half the rate. ----
    const float invT = 1.0f / (float)Tp;
    const int npad = 32 * G;
    float* cstat = reinterpret_cast<float*>(conv_dyn_lds);          // [2][128]; the staging memory is free now
    __syncthreads();                                                // ... once every wave has left its last chunk
    if (EPI == X3_FWD) {
        const float rs = 1.0f / sqrtf(st2 * invT + 1e-5f);
        if (kg == 0) { rstd_clip[col] = rs; cstat[wave * 16 + r16] = st1; cstat[128 + wave * 16 + r16] = rs; }
    } else {
        float s1 = st1, s2 = st2;
        s1 += __shfl_xor(s1, 16);
        s1 += __shfl_xor(s1, 32);
        s2 += __shfl_xor(s2, 16);
        s2 += __shfl_xor(s2, 32);
        if (kg == 0) { cstat[wave * 16 + r16] = s1 * invT; cstat[128 + wave * 16 + r16] = s2 * invT; }
    }
    __syncthreads();                                                // statistics in LDS; every wave's raw rows are visible
    const int c4 = (lane & 31) * 4, rr = 2 * wave + (lane >> 5);
    const float4 q0 = *reinterpret_cast<const float4*>(cstat + c4), q1 = *reinterpret_cast<const float4*>(cstat + 128 + c4);
    float* const Cw = C + (size_t)row0 * ldc + bn + c4;
    float pm = 0.f;                                                 // max |value| of this lane's 4 columns (kScaled)
    if (EPI == X3_FWD) {
        for (int r0 = rr; r0 < npad; r0 += 64) {                    // four rows per lane in flight
            float4 z[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = *reinterpret_cast<const float4*>(Cw + (size_t)min(r0 + 16 * j, npad - 1) * ldc);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = r0 + 16 * j;
                if (r >= npad) continue;
                auto f = [&](float v, float mean, float rs) {
                    const float u = (v - mean) * rs;
                    const float o = (r < Tp) ? (u > 0.f ? u : 0.2f * u) : 0.f;
                    pm = fmaxf(pm, fabsf(o));
                    return o;
                };
                *reinterpret_cast<float4*>(Cw + (size_t)r * ldc) =
                    make_float4(f(z[j].x, q0.x, q1.x), f(z[j].y, q0.y, q1.y), f(z[j].z, q0.z, q1.z), f(z[j].w, q0.w, q1.w));
            }
        }
    } else {
        const float4 rs4 = *reinterpret_cast<const float4*>(rstd_clip + bn + c4);
        const float* const Aw = act + (size_t)row0 * ldc + bn + c4;
        for (int r0 = rr; r0 < npad; r0 += 64) {
            float4 du[4], av[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t o = (size_t)min(r0 + 16 * j, npad - 1) * ldc;
                du[j] = *reinterpret_cast<const float4*>(Cw + o);
                av[j] = *reinterpret_cast<const float4*>(Aw + o);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = r0 + 16 * j;
                if (r >= npad) continue;
                auto f = [&](float d, float a, float rs, float m1, float m2) {
                    const float uv = a > 0.f ? a : a * 5.0f;
                    const float o = (r < Tp) ? rs * (d - m1 - uv * m2) : 0.f;
                    pm = fmaxf(pm, fabsf(o));
                    return o;
                };
                *reinterpret_cast<float4*>(Cw + (size_t)r * ldc) =
                    make_float4(f(du[j].x, av[j].x, rs4.x, q0.x, q1.x), f(du[j].y, av[j].y, rs4.y, q0.y, q1.y),
                                f(du[j].z, av[j].z, rs4.z, q0.z, q1.z), f(du[j].w, av[j].w, rs4.w, q0.w, q1.w));
            }
        }
    }
    if constexpr (P::kScaled) {
        if (amax_out) {
            // the 16-column group of a lane is (lane & 31) >> 2: its four lanes in both half-waves, then the eight waves through LDS
            pm = fmaxf(pm, __shfl_xor(pm, 1));
            pm = fmaxf(pm, __shfl_xor(pm, 2));
            pm = fmaxf(pm, __shfl_xor(pm, 32));
            float* gm = cstat + 256;                                    // [8 waves][8 groups]
            if ((lane & 35) == 0) gm[wave * 8 + ((lane & 31) >> 2)] = pm;
            __syncthreads();
            if (threadIdx.x < 8) {
                float m = 0.f;
#pragma unroll
                for (int w = 0; w < 8; ++w) m = fmaxf(m, gm[w * 8 + threadIdx.x]);
                amax_out[(size_t)clip * 64 + (bn >> 4) + threadIdx.x] = m;
            }
        }
    }
}

}  // namespace aware
