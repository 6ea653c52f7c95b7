// Detector network kernels for gfx950: fp32 MFMA GEMM (1x1 convolutions and the mel
// projection are dense contractions over channels) plus the normalisation /
// activation / read-out kernels and their hand-written backward passes.
//
// Activations are TIME-MAJOR: a clip's frames are consecutive rows and the channel
// dimension is contiguous, [rows][C].  A 1x1 Conv1d (weight [Cout][Cin]) is then
//     Z[rows][Cout] = X[rows][Cin] * W[Cout][Cin]^T
// i.e. an "NT" GEMM whose two operands are both contiguous along the reduction
// dimension, which is what the f32 MFMA fragments want (one ds_read_b128 = four
// k-steps).  The data-gradient uses the pre-transposed weight the same way.
//
// Reference (all under /root/reference/src/AWARE/detection):
//   multibit_detector_net.py:109-140 forward; modules/mel.py:185-201 (mel matmul);
//   modules/conv1d.py:38-42 (conv -> InstanceNorm1d -> LeakyReLU(0.2));
//   modules/globalStandardize.py:16-21; modules/BRH.py:16-27;
//   embedding/losses.py:38-42 (push_extremes) and :12-14,:23-25,:68-70.
#include <mutex>

#include "common.hpp"
#include "kernels.h"
#include "mel_norm.hpp"
#include "mel_chunked.hpp"

namespace aware {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------
// fp32 MFMA GEMM, C = A * Bt^T + bias.
// Template: block tile BM x BN, NWM x NWN waves (each owns (BM/NWM) x (BN/NWN), a grid of
// 32x32 MFMA tiles), K tile BK, DB = number of LDS buffers (1: two barriers per K tile,
// 2: one barrier, next tile written while the current one is consumed).
// LDS rows are padded to BK+4 floats: the 16-lane groups of ds_read_b128 then hit 64
// distinct banks.  Within each group of 8 k, lane half h = lane>>5 takes k = 4h..4h+3
// as four MFMA steps (any k permutation is legal as long as A and B agree).
// ---------------------------------------------------------------------------------
template <int BM, int BN, int NWM, int NWN, int BK, int DB>
__global__ __launch_bounds__(64 * NWM * NWN) void gemm_nt_kernel(const float* __restrict__ A, int lda,
                                                                  const float* __restrict__ Bt, int ldb,
                                                                  const float* __restrict__ bias, float* __restrict__ C,
                                                                  int ldc, int M, int N, int K, int tiles_n, int ntiles,
                                                                  int kchunk) {
    constexpr int NT = 64 * NWM * NWN, LD = BK + 4, KQ = BK / 4;
    constexpr int WM = BM / NWM, WN = BN / NWN, TM = WM / 32, TN = WN / 32;
    constexpr int RPP = NT / KQ;                       // rows covered by one pass of float4 loads
    constexpr int LA = (BM + RPP - 1) / RPP, LB = (BN + RPP - 1) / RPP;
    static_assert(WM % 32 == 0 && WN % 32 == 0 && BK % 8 == 0, "tile shape");
    __shared__ float As[DB][BM * LD];
    __shared__ float Bs[DB][BN * LD];

    // XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs, so give each
    // XCD a contiguous run of tiles (tiles of one row panel share A through that XCD's L2)
    int id = blockIdx.x;
    if ((ntiles & 7) == 0) id = (id & 7) * (ntiles >> 3) + (id >> 3);
    const int bm = (id / tiles_n) * BM;
    const int bn = (id % tiles_n) * BN;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / NWN, wn = wave % NWN;
    const int li = lane & 31, lh = lane >> 5;
    const int lrow = tid / KQ, lkq = (tid % KQ) * 4;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    float4 ra[LA], rb[LB];
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < LA; ++i) {
            int rl = lrow + RPP * i, r = bm + rl, k = k0 + lkq;
            ra[i] = (rl < BM && r < M && k < K) ? *reinterpret_cast<const float4*>(A + (size_t)r * lda + k) : make_float4(0, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < LB; ++i) {
            int rl = lrow + RPP * i, r = bn + rl, k = k0 + lkq;
            rb[i] = (rl < BN && r < N && k < K) ? *reinterpret_cast<const float4*>(Bt + (size_t)r * ldb + k) : make_float4(0, 0, 0, 0);
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < LA; ++i)
            if (lrow + RPP * i < BM) *reinterpret_cast<float4*>(&As[buf][(lrow + RPP * i) * LD + lkq]) = ra[i];
#pragma unroll
        for (int i = 0; i < LB; ++i)
            if (lrow + RPP * i < BN) *reinterpret_cast<float4*>(&Bs[buf][(lrow + RPP * i) * LD + lkq]) = rb[i];
    };
    auto compute = [&](int buf) {
        const float* as = As[buf];
        const float* bs = Bs[buf];
#pragma unroll
        for (int g = 0; g < BK / 8; ++g) {
            float4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                af[i] = *reinterpret_cast<const float4*>(&as[(wm * WM + i * 32 + li) * LD + 8 * g + 4 * lh]);
#pragma unroll
            for (int j = 0; j < TN; ++j)
                bf[j] = *reinterpret_cast<const float4*>(&bs[(wn * WN + j * 32 + li) * LD + 8 * g + 4 * lh]);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].x, bf[j].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].y, bf[j].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].z, bf[j].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].w, bf[j].w, acc[i][j], 0, 0, 0);
                }
        }
    };

    // split-K: blockIdx.y owns k in [kbeg, kend) and writes its own partial slab C + y*M*ldc
    const int kbeg = blockIdx.y * kchunk;
    const int kend = min(K, kbeg + kchunk);
    K = kend;                                            // the loaders zero-fill beyond K
    C += (size_t)blockIdx.y * M * ldc;
    const int nk = (kend - kbeg + BK - 1) / BK;
    gload(kbeg);
    sstore(0);
    if (nk > 1) gload(kbeg + BK);
    __syncthreads();
    if (DB == 2) {
        for (int kt = 0; kt < nk; ++kt) {
            const int cur = kt & 1;
            compute(cur);
            if (kt + 1 < nk) {
                // buffer cur^1 was last read in iteration kt-1, which every wave left through the
                // barrier below; the registers hold tile kt+1
                sstore(cur ^ 1);
                if (kt + 2 < nk) gload(kbeg + (kt + 2) * BK);
            }
            __syncthreads();
        }
    } else {
        for (int kt = 0; kt < nk; ++kt) {
            compute(0);
            __syncthreads();
            if (kt + 1 < nk) {
                sstore(0);
                if (kt + 2 < nk) gload(kbeg + (kt + 2) * BK);
                __syncthreads();
            }
        }
    }
    // C/D layout of the 32x32 MFMA: col = lane&31, row = (e&3) + 8*(e>>2) + 4*(lane>>5)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = bn + wn * WN + j * 32 + li;
            const float bv = (bias && col < N) ? bias[col] : 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = bm + wm * WM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (row < M && col < N) C[(size_t)row * ldc + col] = acc[i][j][e] + bv;
            }
        }
}

template <int BM, int BN, int NWM, int NWN, int BK, int DB>
static void gemm_launch(const float* A, int lda, const float* Bt, int ldb, const float* bias, float* C, int ldc, int M,
                        int N, int K, hipStream_t st, int ksplit = 1) {
    int tn = (N + BN - 1) / BN, tm = (M + BM - 1) / BM;
    int kchunk = ((K + ksplit - 1) / ksplit + BK - 1) / BK * BK;
    hipLaunchKernelGGL((gemm_nt_kernel<BM, BN, NWM, NWN, BK, DB>), dim3(tn * tm, ksplit), dim3(64 * NWM * NWN), 0, st, A, lda,
                       Bt, ldb, bias, C, ldc, M, N, K, tn, tn * tm, kchunk);
}

// split-K variant for skinny outputs (N <= 64): ksplit partial slabs C[z][M][ldc], no bias
void launch_gemm_nt_splitk(const float* A, int lda, const float* Bt, int ldb, float* Cpart, int ldc, int M, int N, int K,
                           int ksplit, hipStream_t st) {
    gemm_launch<64, 64, 2, 2, 32, 1>(A, lda, Bt, ldb, nullptr, Cpart, ldc, M, N, K, st, ksplit);
}

// ---------------------------------------------------------------------------------
// Clip-aligned GEMM with the conv block's tail fused into the epilogue.
// Pooled rows are laid out 32-aligned per clip; for a uniform batch whose clips need
// NWM <= 4 groups of 32 rows, one workgroup owns ALL rows of one clip for a 32*NWN-column
// slab, so the per-(clip, channel) InstanceNorm statistics are complete inside the
// workgroup:
//   EPI_FWD: C = LeakyReLU_0.2((z - mean_t z) * rstd), z = acc + bias; rstd saved
//            (modules/conv1d.py:38-42: conv -> InstanceNorm1d -> LeakyReLU)
//   EPI_BWD: acc = dL/dA of the PREVIOUS block's output A (read here, post-activation);
//            C = dL/dZ = rstd * (dU - mean_t dU - u * mean_t(dU*u)), dU = acc * lrelu'(u)
// This removes the separate normalisation passes (one read + one write of the activation each).
// Same main loop as gemm_nt_kernel, wave tile 32x32, BK = 32, one LDS buffer.
// ---------------------------------------------------------------------------------
enum { EPI_PLAIN = 0, EPI_FWD = 1, EPI_BWD = 2 };

// Epilogue shared by the clip-aligned GEMM kernels: the wave holds rows
// wm*32 + (e&3) + 8*(e>>2) + 4*lh of column `col` of clip `clip` (see gemm_clip_kernel).
template <int NWM, int NWN, int EPI>
__device__ __forceinline__ void clip_epilogue(const f32x16& acc, float (*red1)[32 * NWN], float (*red2)[32 * NWN], int wm,
                                              int wn, int li, int lh, int clip, int bm, int bn, int Tp, int N, int ldc,
                                              const float* __restrict__ bias, float* __restrict__ C,
                                              float* __restrict__ rstd_io, const float* __restrict__ act) {
    // ---- epilogue: this wave holds rows wm*32 + (e&3) + 8*(e>>2) + 4*lh of column col ----
    const int cl = wn * 32 + li;             // column inside the slab
    const int col = bn + cl;
    const bool cok = col < N;
    const float invT = 1.0f / (float)Tp;
    if (EPI == EPI_PLAIN) {
        const float bv = (bias && cok) ? bias[col] : 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
            if (cok) C[(size_t)(bm + r) * ldc + col] = (r < Tp) ? acc[e] + bv : 0.f;
        }
        return;
    }
    if (EPI == EPI_FWD) {
        const float bv = (bias && cok) ? bias[col] : 0.f;
        float z[16];
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
            z[e] = acc[e] + bv;
            if (r < Tp) s += z[e];
        }
        s += __shfl_xor(s, 32);
        if (lh == 0) red1[wm][cl] = s;
        __syncthreads();
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < NWM; ++w) tot += red1[w][cl];
        const float mean = tot * invT;
        float q = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
            if (r < Tp) { const float d = z[e] - mean; q += d * d; }
        }
        q += __shfl_xor(q, 32);
        if (lh == 0) red2[wm][cl] = q;
        __syncthreads();
        float qt = 0.f;
#pragma unroll
        for (int w = 0; w < NWM; ++w) qt += red2[w][cl];
        const float rs = 1.0f / sqrtf(qt * invT + 1e-5f);
        if (cok && wm == 0 && lh == 0) rstd_io[(size_t)clip * N + col] = rs;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
            const float u = (z[e] - mean) * rs;
            if (cok) C[(size_t)(bm + r) * ldc + col] = (r < Tp) ? (u > 0.f ? u : 0.2f * u) : 0.f;
        }
        return;
    }
    // EPI_BWD
    {
        const float rs = cok ? rstd_io[(size_t)clip * N + col] : 0.f;
        float du[16], u[16];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
            // loaded for every row of the 32-row groups (padding rows exist and hold zeros): a per-element branch
            // would serialise the loads behind their waits
            const float av = act[(size_t)(bm + r) * ldc + (cok ? col : 0)];
            const bool valid = cok && r < Tp;
            u[e] = valid ? (av > 0.f ? av : av * 5.0f) : 0.f;                 // invert LeakyReLU(0.2)
            du[e] = valid ? acc[e] * (av > 0.f ? 1.f : 0.2f) : 0.f;
            s1 += du[e]; s2 += du[e] * u[e];
        }
        s1 += __shfl_xor(s1, 32);
        s2 += __shfl_xor(s2, 32);
        if (lh == 0) { red1[wm][cl] = s1; red2[wm][cl] = s2; }
        __syncthreads();
        float t1 = 0.f, t2 = 0.f;
#pragma unroll
        for (int w = 0; w < NWM; ++w) { t1 += red1[w][cl]; t2 += red2[w][cl]; }
        const float m1 = t1 * invT, m2 = t2 * invT;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
            if (cok) C[(size_t)(bm + r) * ldc + col] = (r < Tp) ? rs * (du[e] - m1 - u[e] * m2) : 0.f;
        }
    }
}


template <int NWM, int NWN, int EPI, int BK, int DB, bool EXACT>
__global__ __launch_bounds__(64 * NWM * NWN) void gemm_clip_kernel(const float* __restrict__ A, int lda,
                                                                    const float* __restrict__ Bt, int ldb,
                                                                    const float* __restrict__ bias, float* __restrict__ C,
                                                                    int ldc, int Tp, int N, int K, int tiles_n, int ntiles,
                                                                    float* __restrict__ rstd_io,
                                                                    const float* __restrict__ act) {
    constexpr int BM = 32 * NWM, BN = 32 * NWN;
    constexpr int NT = 64 * NWM * NWN, LD = BK + 4, KQ = BK / 4;
    constexpr int RPP = NT / KQ;
    constexpr int LA = (BM + RPP - 1) / RPP, LB = (BN + RPP - 1) / RPP;
    __shared__ float As[DB][BM * LD];
    __shared__ float Bs[DB][BN * LD];
    __shared__ float red1[NWM][BN], red2[NWM][BN];

    int id = blockIdx.x;
    if ((ntiles & 7) == 0) id = (id & 7) * (ntiles >> 3) + (id >> 3);
    const int clip = id / tiles_n;
    const int bm = clip * BM;
    const int bn = (id % tiles_n) * BN;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / NWN, wn = wave % NWN;
    const int li = lane & 31, lh = lane >> 5;
    const int lrow = tid / KQ, lkq = (tid % KQ) * 4;

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;

    float4 ra[LA], rb[LB];
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < LA; ++i) {
            int rl = lrow + RPP * i, k = k0 + lkq;
            // EXACT: K % BK == 0 and N % BN == 0, so only the static row-count guard remains
            const bool ok = (BM % RPP == 0 || rl < BM) && (EXACT || k < K);
            ra[i] = ok ? *reinterpret_cast<const float4*>(A + (size_t)(bm + rl) * lda + k) : make_float4(0, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < LB; ++i) {
            int rl = lrow + RPP * i, r = bn + rl, k = k0 + lkq;
            const bool ok = (BN % RPP == 0 || rl < BN) && (EXACT || (r < N && k < K));
            rb[i] = ok ? *reinterpret_cast<const float4*>(Bt + (size_t)r * ldb + k) : make_float4(0, 0, 0, 0);
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < LA; ++i)
            if (lrow + RPP * i < BM) *reinterpret_cast<float4*>(&As[buf][(lrow + RPP * i) * LD + lkq]) = ra[i];
#pragma unroll
        for (int i = 0; i < LB; ++i)
            if (lrow + RPP * i < BN) *reinterpret_cast<float4*>(&Bs[buf][(lrow + RPP * i) * LD + lkq]) = rb[i];
    };
    auto compute = [&](int buf) {
#pragma unroll
        for (int g = 0; g < BK / 8; ++g) {
            const float4 af = *reinterpret_cast<const float4*>(&As[buf][(wm * 32 + li) * LD + 8 * g + 4 * lh]);
            const float4 bf = *reinterpret_cast<const float4*>(&Bs[buf][(wn * 32 + li) * LD + 8 * g + 4 * lh]);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, bf.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, bf.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, bf.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, bf.w, acc, 0, 0, 0);
        }
    };
    const int nk = (K + BK - 1) / BK;
    if (DB == 2) {
        gload(0);
        sstore(0);
        if (nk > 1) gload(BK);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int cur = kt & 1;
            compute(cur);
            if (kt + 1 < nk) {
                sstore(cur ^ 1);
                if (kt + 2 < nk) gload((kt + 2) * BK);
            }
            __syncthreads();
        }
    } else {
        // one LDS buffer, TWO register sets: the loads of K tile kt+2 and kt+3 are in flight while tile kt
        // is consumed, so a load has two tile periods to land before its s_waitcnt (two tiles per trip to
        // keep the register sets statically indexed)
        float4 ra2[LA], rb2[LB];
        auto gload2 = [&](int k0) {
#pragma unroll
            for (int i = 0; i < LA; ++i) {
                int rl = lrow + RPP * i, k = k0 + lkq;
                const bool ok = (BM % RPP == 0 || rl < BM) && (EXACT || k < K);
                ra2[i] = ok ? *reinterpret_cast<const float4*>(A + (size_t)(bm + rl) * lda + k) : make_float4(0, 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < LB; ++i) {
                int rl = lrow + RPP * i, r = bn + rl, k = k0 + lkq;
                const bool ok = (BN % RPP == 0 || rl < BN) && (EXACT || (r < N && k < K));
                rb2[i] = ok ? *reinterpret_cast<const float4*>(Bt + (size_t)r * ldb + k) : make_float4(0, 0, 0, 0);
            }
        };
        auto sstore2 = [&]() {
#pragma unroll
            for (int i = 0; i < LA; ++i)
                if (lrow + RPP * i < BM) *reinterpret_cast<float4*>(&As[0][(lrow + RPP * i) * LD + lkq]) = ra2[i];
#pragma unroll
            for (int i = 0; i < LB; ++i)
                if (lrow + RPP * i < BN) *reinterpret_cast<float4*>(&Bs[0][(lrow + RPP * i) * LD + lkq]) = rb2[i];
        };
        gload(0);
        sstore(0);
        if (nk > 1) gload(BK);            // set 1 <- tile 1
        if (nk > 2) gload2(2 * BK);       // set 2 <- tile 2
        __syncthreads();
        for (int kt = 0; kt < nk; kt += 2) {
            compute(0);                                   // tile kt
            __syncthreads();
            if (kt + 1 < nk) {
                sstore(0);                                // tile kt+1 (set 1)
                if (kt + 3 < nk) gload((kt + 3) * BK);    // set 1 <- tile kt+3
                __syncthreads();
                compute(0);                               // tile kt+1
                __syncthreads();
                if (kt + 2 < nk) {
                    sstore2();                            // tile kt+2 (set 2)
                    if (kt + 4 < nk) gload2((kt + 4) * BK);   // set 2 <- tile kt+4
                    __syncthreads();
                }
            }
        }
    }

    clip_epilogue<NWM, NWN, EPI>(acc, red1, red2, wm, wn, li, lh, clip, bm, bn, Tp, N, ldc, bias, C, rstd_io, act);
}

template <int NWM, int NWN, int EPI, int BK, int DB>
static void clip_launch(const float* A, int lda, const float* Bt, int ldb, const float* bias, float* C, int ldc, int B,
                        int Tp, int N, int K, float* rstd_io, const float* act, hipStream_t st) {
    const int tn = (N + 32 * NWN - 1) / (32 * NWN);
    if (K % BK == 0 && N % (32 * NWN) == 0)
        hipLaunchKernelGGL((gemm_clip_kernel<NWM, NWN, EPI, BK, DB, true>), dim3(tn * B), dim3(64 * NWM * NWN), 0, st, A, lda, Bt,
                           ldb, bias, C, ldc, Tp, N, K, tn, tn * B, rstd_io, act);
    else
        hipLaunchKernelGGL((gemm_clip_kernel<NWM, NWN, EPI, BK, DB, false>), dim3(tn * B), dim3(64 * NWM * NWN), 0, st, A, lda, Bt,
                           ldb, bias, C, ldc, Tp, N, K, tn, tn * B, rstd_io, act);
}

// rows_per_clip = 32 * nwm (1..4).  epi: 0 plain, 1 forward IN+LeakyReLU, 2 backward of IN+LeakyReLU.
// The f32-MFMA kernel (BK 32, one LDS buffer, two-deep register prefetch): aware_embed_config.conv_pipe = 1 and the
// shapes the bf16x3 kernel (gemm_x3.hip) does not serve.
void launch_gemm_clip(const float* A, int lda, const float* Bt, int ldb, const float* bias, float* C, int ldc, int B,
                      int nwm, int Tp, int N, int K, int epi, float* rstd_io, const float* act, hipStream_t st) {
#define CL(M_, E_, K_, D_) clip_launch<M_, 4, E_, K_, D_>(A, lda, Bt, ldb, bias, C, ldc, B, Tp, N, K, rstd_io, act, st)
#define CLM(E_, K_, D_)                                                                                            \
    switch (nwm) { case 1: CL(1, E_, K_, D_); break; case 2: CL(2, E_, K_, D_); break; case 3: CL(3, E_, K_, D_); break; \
                   default: CL(4, E_, K_, D_); break; }
#define CLE(K_, D_)                                   \
    if (epi == EPI_FWD) { CLM(EPI_FWD, K_, D_) }      \
    else if (epi == EPI_BWD) { CLM(EPI_BWD, K_, D_) } \
    else { CLM(EPI_PLAIN, K_, D_) }
    CLE(32, 1)
#undef CLE
#undef CLM
#undef CL
}

// Tile configurations.  All of them accumulate k in the same order, so the result of a GEMM
// is bit-identical whichever one runs: choosing by measurement does not change numerics.
constexpr int kNumGemmVariants = 12;   // variants above this number are experiments, not auto-tuned
static void gemm_dispatch(int variant, const float* A, int lda, const float* Bt, int ldb, const float* bias, float* C,
                          int ldc, int M, int N, int K, hipStream_t st) {
#define GL(...) gemm_launch<__VA_ARGS__>(A, lda, Bt, ldb, bias, C, ldc, M, N, K, st)
    switch (variant) {
        case 1: GL(128, 128, 2, 2, 32, 1); break;
        case 2: GL(128, 64, 2, 2, 32, 1); break;
        case 3: GL(64, 64, 2, 2, 32, 2); break;
        case 4: GL(64, 64, 2, 2, 32, 1); break;
        case 5: GL(64, 64, 2, 2, 16, 2); break;
        case 6: GL(64, 64, 2, 2, 64, 1); break;
        case 7: GL(64, 128, 2, 2, 32, 1); break;
        case 8: GL(128, 128, 4, 2, 16, 2); break;
        case 9: GL(96, 64, 3, 2, 32, 1); break;
        case 10: GL(128, 64, 4, 2, 32, 1); break;
        case 11: GL(64, 128, 2, 4, 32, 1); break;
        case 12: GL(128, 128, 4, 4, 32, 1); break;
        case 13: GL(96, 128, 3, 4, 32, 1); break;
        case 14: GL(96, 128, 3, 4, 16, 2); break;
        case 15: GL(96, 64, 3, 2, 16, 2); break;
        case 16: GL(96, 128, 3, 4, 32, 2); break;
        default: GL(64, 64, 2, 2, 32, 1); break;
    }
#undef GL
}

// measured choice per shape (filled by gemm_autotune, e.g. from aware_embed_create).  A memo only: every
// configuration gives bit-identical results, so the cache never changes what a call computes; guarded by a
// mutex so that sessions may be created from several host threads.
struct GemmChoice { int M, N, K, variant; };
static GemmChoice g_choice[64];
static int g_nchoice = 0;
static std::mutex g_choice_mu;

static int gemm_heuristic(int M, int N, int K) {
    if (N <= 64) return 6;
    if (K <= 64) return 5;
    long t = (long)((M + 127) / 128) * ((N + 63) / 64);
    return (t >= 700) ? 10 : 4;
}
static int gemm_lookup(int M, int N, int K) {
    std::lock_guard<std::mutex> lk(g_choice_mu);
    for (int i = 0; i < g_nchoice; ++i)
        if (g_choice[i].M == M && g_choice[i].N == N && g_choice[i].K == K) return g_choice[i].variant;
    return 0;
}

// Time every configuration on this shape (operands are scratch memory, contents irrelevant)
// and remember the fastest.  Synchronises the stream; call outside graph capture.
int gemm_autotune(const float* A, int lda, const float* Bt, int ldb, float* C, int ldc, int M, int N, int K,
                  hipStream_t st) {
    if (gemm_lookup(M, N, K)) return gemm_lookup(M, N, K);
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return gemm_heuristic(M, N, K);
    int best = gemm_heuristic(M, N, K);
    float best_ms = 1e30f;
    for (int v = 1; v <= kNumGemmVariants; ++v) {
        if (N <= 64 && (v == 1 || v == 7 || v == 8 || v == 11 || v == 12)) continue;     // >= 128-wide tiles
        gemm_dispatch(v, A, lda, Bt, ldb, nullptr, C, ldc, M, N, K, st);                    // warm-up
        (void)hipEventRecord(e0, st);
        for (int r = 0; r < 4; ++r) gemm_dispatch(v, A, lda, Bt, ldb, nullptr, C, ldc, M, N, K, st);
        (void)hipEventRecord(e1, st);
        if (hipEventSynchronize(e1) != hipSuccess) break;
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        if (ms < best_ms) { best_ms = ms; best = v; }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    {
        std::lock_guard<std::mutex> lk(g_choice_mu);
        if (g_nchoice < 64) g_choice[g_nchoice++] = GemmChoice{M, N, K, best};
    }
    return best;
}

// variant: 0 = automatic (measured choice if the shape was tuned, else a heuristic)
void launch_gemm_nt_variant(const float* A, int lda, const float* Bt, int ldb, const float* bias, float* C, int ldc,
                            int M, int N, int K, int variant, hipStream_t st) {
    if (variant == 0) {
        variant = gemm_lookup(M, N, K);
        if (!variant) variant = gemm_heuristic(M, N, K);
    }
    gemm_dispatch(variant, A, lda, Bt, ldb, bias, C, ldc, M, N, K, st);
}

void launch_gemm_nt(const float* A, int lda, const float* Bt, int ldb, const float* bias, float* C, int ldc, int M,
                    int N, int K, hipStream_t st) {
    launch_gemm_nt_variant(A, lda, Bt, ldb, bias, C, ldc, M, N, K, 0, st);
}

// ---------------------------------------------------------------------------------
// block reductions
// ---------------------------------------------------------------------------------
// (wave_partials and the 256-thread block_sum: mel_chunked.hpp)
// 512 threads
__device__ __forceinline__ float mel_block_sum(float v, float* red8) {
    wave_partials(v, red8);
    return mel_sum8(red8);
}

// ---------------------------------------------------------------------------------
// mel block (the maths: mel_norm.hpp), chunked form, for clips longer than kMelClipFrames.  Time is cut into 32-frame chunks
// so that B * ceil(T/32) workgroups share the work; per-channel statistics are produced as per-chunk (count, mean, M2)
// partials and merged with Chan's formula by every consumer workgroup in fixed order (deterministic, no atomics).
// Partials [B][pstride][2 Mp] = {mean | D1, M2 | D2} per chunk.
//
// One family for every bank of n_mels <= 512 bands in rows of Mp >= n_mels floats (Mp a multiple of 4; stored_channels in
// capi.hip): channels are taken in groups of 128 (thread c of a group: channel 128 j + c, row group g: every second row), and
// the clip-wide GlobalStandardize sum runs over the n_mels real channels only.  Padding channels n_mels .. Mp-1 get zero
// statistics, zero x0 columns and zero dL/dxm.  MelBank128 makes the card's 128 bands, pitch and single group compile-time
// constants; MelBankAny takes them at run time.  Row loops have a fixed trip count, loads first (clamped indices), stores
// masked: no per-iteration load/wait chain.
// ---------------------------------------------------------------------------------
// (MelBank128 and MelBankAny: mel_chunked.hpp, shared with the pooled nets' kernels of mel_pool_kernels.hip)

// per-chunk (mean, M2) of every channel
template <class Bank>
__global__ __launch_bounds__(256) void mel_partial_stats_kernel(const float* __restrict__ xm, const int* __restrict__ frame_off,
                                                                 float* __restrict__ part, int pstride, int n_mels, int Mp) {
    __shared__ float s1[2][128];
    const Bank bk(n_mels, Mp);
    const int b = blockIdx.y;
    const int f0 = frame_off[b], T = frame_off[b + 1] - f0;
    const int t0 = blockIdx.x * kMelChunk;
    if (t0 >= T) return;
    const int nt = min(kMelChunk, T - t0);
    const int c = threadIdx.x & 127, g = threadIdx.x >> 7;
    float* o = part + ((size_t)b * pstride + blockIdx.x) * 2 * bk.Mp;
    for (int j = 0; j < bk.ng; ++j) {
        const int ch = 128 * j + c;
        const bool on = ch < bk.n_mels;
        const float* x = xm + (size_t)(f0 + t0) * bk.Mp + min(ch, bk.n_mels - 1);
        float v[kMelChunk / 2];
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < kMelChunk / 2; ++i) {
            const int t = 2 * i + g;
            v[i] = (t < nt) ? x[(size_t)t * bk.Mp] : 0.f;
            a += v[i];
        }
        s1[g][c] = a;
        __syncthreads();
        const float mean = (s1[0][c] + s1[1][c]) / (float)nt;
        __syncthreads();
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < kMelChunk / 2; ++i) {
            const int t = 2 * i + g;
            if (t < nt) { float d = v[i] - mean; q += d * d; }
        }
        s1[g][c] = q;
        __syncthreads();
        if (g == 0 && ch < bk.Mp) {
            o[ch] = on ? mean : 0.f;
            o[bk.Mp + ch] = on ? s1[0][c] + s1[1][c] : 0.f;
        }
        if (Bank::kGroups > 1) __syncthreads();
    }
}

template <class Bank>
__global__ __launch_bounds__(256) void mel_apply_pool_kernel(const float* __restrict__ xm, const int* __restrict__ frame_off,
                                                              const int* __restrict__ pool_off, const float* __restrict__ part,
                                                              int pstride, float* __restrict__ x0, float* __restrict__ stats,
                                                              float* __restrict__ gstat, int n_mels, int Mp) {
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
    // pooled frames tp = t0/2 .. ; chunk is even-sized so pairs never straddle chunks
    const int Tp = T / 2;
    const int tp0 = t0 / 2, tp1 = min(Tp, tp0 + kMelChunk / 2);
    const bool last = (int)blockIdx.x == nchunk - 1;
#pragma unroll
    for (int j = 0; j < Bank::kGroups; ++j) {
        const int ch = 128 * j + c;
        if (j >= bk.ng || ch >= bk.Mp) continue;
        const bool on = ch < bk.n_mels;
        if (blockIdx.x == 0 && g == 0) mel_write_stats(stats, (size_t)b * bk.Mp + ch, mus[j], rss[j], M2s[j]);
        const float* x = xm + (size_t)f0 * bk.Mp + ch;
        float* o = x0 + (size_t)pool_off[b] * bk.Mp + ch;
        const float mu = mus[j], rs = rss[j];
        if (Tp > 0) {
            constexpr int NI = kMelChunk / 4;
            float xa[NI], xb[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int tc = min(tp0 + g + 2 * i, Tp - 1);
                xa[i] = x[(size_t)(2 * tc) * bk.Mp];
                xb[i] = x[(size_t)(2 * tc + 1) * bk.Mp];
            }
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int tp = tp0 + g + 2 * i;
                if (tp < tp1)                                         // padding channels stay zero
                    o[(size_t)tp * bk.Mp] = on ? mel_pooled(mel_u(xa[i], mu, rs), mel_u(xb[i], mu, rs), k.ginv) : 0.f;
            }
        }
        // pooled rows are 32-aligned per clip: keep the pad rows finite (they flow through the GEMMs)
        if (last)
            for (int tp = Tp + g; tp < ((Tp + 31) & ~31); tp += 2) o[(size_t)tp * bk.Mp] = 0.f;
    }
}

// backward partials: D1_c = sum_t dv, D2_c = sum_t dv*u over the chunk (dv = dx0/2 on pooled frames)
template <class Bank>
__global__ __launch_bounds__(256) void mel_bwd_partial_kernel(const float* __restrict__ dx0, const float* __restrict__ xm,
                                                               const int* __restrict__ frame_off, const int* __restrict__ pool_off,
                                                               const float* __restrict__ stats, float* __restrict__ part,
                                                               int pstride, int n_mels, int Mp) {
    __shared__ float s1[2][128], s2[2][128];
    const Bank bk(n_mels, Mp);
    const int b = blockIdx.y;
    const int f0 = frame_off[b], T = frame_off[b + 1] - f0, Tp = T / 2;
    const int t0 = blockIdx.x * kMelChunk;
    if (t0 >= T) return;
    const int c = threadIdx.x & 127, g = threadIdx.x >> 7;
    const int tp0 = t0 / 2, tp1 = min(Tp, tp0 + kMelChunk / 2);
    float* o = part + ((size_t)b * pstride + blockIdx.x) * 2 * bk.Mp;
    for (int j = 0; j < bk.ng; ++j) {
        const int ch = 128 * j + c;
        const bool on = ch < bk.n_mels;
        const int cc = min(ch, bk.n_mels - 1);
        const MelChan s = mel_read_stats(stats, (size_t)b * bk.Mp + cc);
        const float* x = xm + (size_t)f0 * bk.Mp + cc;
        const float* d0 = dx0 + (size_t)pool_off[b] * bk.Mp + cc;
        float a1 = 0.f, a2 = 0.f;
        if (Tp > 0) {
            constexpr int NI = kMelChunk / 4;
            float dd[NI], xa[NI], xb[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int tc = min(tp0 + g + 2 * i, Tp - 1);
                dd[i] = d0[(size_t)tc * bk.Mp];
                xa[i] = x[(size_t)(2 * tc) * bk.Mp];
                xb[i] = x[(size_t)(2 * tc + 1) * bk.Mp];
            }
#pragma unroll
            for (int i = 0; i < NI; ++i)
                if (tp0 + g + 2 * i < tp1) {
                    const float dv = 0.5f * dd[i];
                    const float u0 = mel_u(xa[i], s.mu, s.rs), u1 = mel_u(xb[i], s.mu, s.rs);
                    a1 += 2.f * dv;
                    a2 += mel_dv_u(dv, u0, u1);
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
__global__ __launch_bounds__(256) void mel_bwd_apply_kernel(const float* __restrict__ dx0, float* __restrict__ xm,
                                                             const int* __restrict__ frame_off, const int* __restrict__ pool_off,
                                                             const float* __restrict__ stats, const float* __restrict__ gstat,
                                                             const float* __restrict__ part, int pstride, int n_mels, int Mp) {
    __shared__ float red[4];
    const Bank bk(n_mels, Mp);
    const int b = blockIdx.y;
    const int f0 = frame_off[b], T = frame_off[b + 1] - f0, Tp = T / 2;
    const int t0 = blockIdx.x * kMelChunk;
    if (t0 >= T) return;
    const int nchunk = (T + kMelChunk - 1) / kMelChunk;
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
        float dd[NI], xv[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int tc = min(t0 + g + 2 * i, T - 1);
            dd[i] = d0[(size_t)min(tc >> 1, max(Tp - 1, 0)) * bk.Mp];
            xv[i] = x[(size_t)tc * bk.Mp];
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int t = t0 + g + 2 * i;
            if (t < t1) {
                const float dv = (t < 2 * Tp) ? 0.5f * dd[i] : 0.f;
                x[(size_t)t * bk.Mp] = mel_bwd_value(dv, mel_u(xv[i], s.mu, s.rs), s.rs, k.ginv, q, m);
            }
        }
    }
}

// ---------------------------------------------------------------------------------
// Conv block tail: the block's norm over time and its activation, in place, and their backward.  The activation, its
// derivative (torch's values at the kinks: ReLU'(0) = 0, LeakyReLU'(0) = 0.2) and the norm are a compile-time policy
// (modules/conv1d.py:8-36, multibit_detector_net.py:82-96).  The model card's blocks are <kNormInstance, kActLRelu>:
// InstanceNorm1d over time (biased var, eps 1e-5) + LeakyReLU(0.2); the fused GEMM epilogues serve those alone.
// ---------------------------------------------------------------------------------
// a * b rounded to float before any use, never fused into a following add or subtract.  The from-memory backward kernel
// computes dL/du in both of its sweeps; fused into `du - m1` the second sweep would see the unrounded product, and a clip of
// one pooled frame (m1 == du, gradient exactly 0) would get the rounding residue of the product instead of 0.  Its other two
// products are written out as well (the sum of du * u from rounded products, u * m2 fused into the subtraction): left to the
// compiler, the pairing of a row's two products into one packed multiply decides which of them is fused, and the pairing moves
// with the shape of the loop around it.
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

template <int ACT>
__device__ __forceinline__ float act_fwd(float u) {
    if (ACT == kActRelu) return u > 0.f ? u : 0.f;
    if (ACT == kActLRelu) return u > 0.f ? u : 0.2f * u;
    if (ACT == kActGelu) return 0.5f * u * (1.f + erff(u * 0.70710678118654752f));      // exact GELU (approximate='none')
    if (ACT == kActSwish) return u / (1.f + expf(-u));                                   // SiLU
    if (ACT == kActTanh) return tanhf(u);
    return 1.f / (1.f + expf(-u));                                                       // sigmoid
}
// f'(u); a = f(u)
template <int ACT>
__device__ __forceinline__ float act_grad(float u, float a) {
    if (ACT == kActRelu) return u > 0.f ? 1.f : 0.f;
    if (ACT == kActLRelu) return u > 0.f ? 1.f : 0.2f;
    if (ACT == kActGelu)
        return 0.5f * (1.f + erff(u * 0.70710678118654752f)) + u * 0.39894228040143268f * expf(-0.5f * u * u);
    if (ACT == kActSwish) {
        const float s = 1.f / (1.f + expf(-u));
        return s * (1.f + u * (1.f - s));
    }
    if (ACT == kActTanh) return 1.f - a * a;
    return a * (1.f - a);
}

// In place: u = norm(z), z = act(u), u -> stash (if given).  Workgroup = (64 channels) x (4 row groups) of one clip.
// R > 0: InstanceNorm with the clip's column in registers (clips of up to 4 R pooled frames: the activation is read once and
// written once); R = 0: from memory (any length; the only form of the element-wise norms).  RULE: kRowsTaps, the rows are those
// of a block of temporal convolutions (TapRows); kRowsPool, those behind an initial pool other than (2, 2) as well; kRowsHalf,
// the kernel never looks at `rows` -- the rule costs registers.
template <int NORM, int ACT, int R, int RULE>
__global__ __launch_bounds__(256) void norm_act_fwd_kernel(float* __restrict__ z, const int* __restrict__ frame_off,
                                                           const int* __restrict__ pool_off, float* __restrict__ rstd,
                                                           const float* __restrict__ scale, const float* __restrict__ shift,
                                                           float* __restrict__ stash, int C, TapRows rows) {
    __shared__ float s[4][64];
    const int b = blockIdx.y, c0 = blockIdx.x * 64;
    const int L0 = rows_l0<RULE>(frame_off[b + 1] - frame_off[b], rows);
    const int r0 = pool_off[b], Tp = RULE != kRowsHalf ? rows.of(L0) : L0;   // rows are 32-aligned per clip
    const int cl = threadIdx.x & 63, g = threadIdx.x >> 6, c = c0 + cl;
    if (Tp <= 0) return;
    const bool ok = c < C;
    float* x = z + (size_t)r0 * C + c;
    // (a block that needs no stash never gets one: for those the rows' stores carry no test)
    float* sx = (norm_act_needs_stash(NORM, ACT) && stash) ? stash + (size_t)r0 * C + c : nullptr;
    float v[R > 0 ? R : 1];
    float mu = 0.f, rs = 1.f, sc = 1.f, sh = 0.f;
    if (NORM == kNormInstance) {
        float a = 0.f;
        if (R > 0) {
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const int t = g + 4 * i;
                v[i] = (ok && t < Tp) ? x[(size_t)t * C] : 0.f;
                a += v[i];
            }
        } else if (ok) {
            for (int t = g; t < Tp; t += 4) a += x[(size_t)t * C];
        }
        s[g][cl] = a;
        __syncthreads();
        mu = (s[0][cl] + s[1][cl] + s[2][cl] + s[3][cl]) / (float)Tp;
        __syncthreads();
        float q = 0.f;
        if (R > 0) {
#pragma unroll
            for (int i = 0; i < R; ++i)
                if (g + 4 * i < Tp) { const float d = v[i] - mu; q += d * d; }
        } else if (ok) {
            for (int t = g; t < Tp; t += 4) { const float d = x[(size_t)t * C] - mu; q += d * d; }
        }
        s[g][cl] = q;
        __syncthreads();
        rs = 1.0f / sqrtf((s[0][cl] + s[1][cl] + s[2][cl] + s[3][cl]) / (float)Tp + 1e-5f);
        if (ok && g == 0) rstd[(size_t)b * C + c] = rs;
    } else if (NORM == kNormAffine) {
        if (ok) { sc = scale[c]; sh = shift[c]; }
    }
    if (!ok) return;
    auto apply = [&](float zv, int t) {
        const float u = NORM == kNormInstance ? (zv - mu) * rs : (NORM == kNormAffine ? zv * sc + sh : zv);
        if (sx) sx[(size_t)t * C] = u;
        x[(size_t)t * C] = act_fwd<ACT>(u);
    };
    if (NORM == kNormInstance && R > 0) {
#pragma unroll
        for (int i = 0; i < R; ++i)
            if (g + 4 * i < Tp) apply(v[i], g + 4 * i);
    } else {
        for (int t = g; t < Tp; t += 4) apply(x[(size_t)t * C], t);
    }
}

// backward of norm_act_fwd_kernel, in place on dA.  u from the stash where the block keeps one (norm_act_needs_stash, a
// function of the policy alone), else from the output A: LeakyReLU inverted; ReLU after an element-wise norm as it is, since
// its derivative only needs the sign of u.
template <int NORM, int ACT, int R, int RULE>
__global__ __launch_bounds__(256) void norm_act_bwd_kernel(float* __restrict__ dA, const float* __restrict__ A,
                                                           const float* __restrict__ stash, const int* __restrict__ frame_off,
                                                           const int* __restrict__ pool_off, const float* __restrict__ rstd,
                                                           const float* __restrict__ scale, int C, TapRows rows) {
    constexpr bool kStash = norm_act_needs_stash(NORM, ACT);
    __shared__ float s1[4][64], s2[4][64];
    const int b = blockIdx.y, c0 = blockIdx.x * 64;
    const int L0 = rows_l0<RULE>(frame_off[b + 1] - frame_off[b], rows);
    const int r0 = pool_off[b], Tp = RULE != kRowsHalf ? rows.of(L0) : L0;   // rows are 32-aligned per clip
    const int cl = threadIdx.x & 63, g = threadIdx.x >> 6, c = c0 + cl;
    if (Tp <= 0) return;
    const bool ok = c < C;
    const int cc = (R > 0 && !ok) ? C - 1 : c;      // the register form loads in every lane, from a clamped column
    float* d = dA + (size_t)r0 * C + cc;
    const float* a = (kStash ? stash : A) + (size_t)r0 * C + cc;
    // (u, f'(u)) from the value v kept at a row.  LeakyReLU's output has the sign of u: one test inverts it and picks the slope
    auto kept = [](float v, float& u, float& slope) {
        if (!kStash && ACT == kActLRelu) {
            const bool pos = v > 0.f;
            u = pos ? v : v * 5.0f;
            slope = pos ? 1.f : 0.2f;
        } else {
            u = v;
            slope = act_grad<ACT>(u, 0.f);
        }
    };
    // (u, dL/du) at row t, from memory
    auto load = [&](int t, float& u, float& du) {
        float slope;
        kept(a[(size_t)t * C], u, slope);
        // (the from-memory InstanceNorm form runs this in both sweeps: see mul_rounded)
        du = (NORM == kNormInstance && R == 0) ? mul_rounded(d[(size_t)t * C], slope) : d[(size_t)t * C] * slope;
    };
    if (NORM != kNormInstance) {
        if (!ok) return;
        const float sc = NORM == kNormAffine ? scale[c] : 1.f;
        for (int t = g; t < Tp; t += 4) {
            float u, du;
            load(t, u, du);
            d[(size_t)t * C] = NORM == kNormAffine ? sc * du : du;
        }
        return;
    }
    float uu[R > 0 ? R : 1], dd[R > 0 ? R : 1];
    float p1 = 0.f, p2 = 0.f;
    if (R > 0) {
        // loads from clamped indices, masked afterwards: a load inside a per-row branch waits for its own latency
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int t = g + 4 * i;
            const int tc = t < Tp ? t : Tp - 1;
            uu[i] = a[(size_t)tc * C];
            dd[i] = d[(size_t)tc * C];
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const bool valid = ok && g + 4 * i < Tp;
            float u, slope;
            kept(uu[i], u, slope);
            uu[i] = valid ? u : 0.f;
            dd[i] = valid ? dd[i] * slope : 0.f;
            p1 += dd[i]; p2 += dd[i] * uu[i];
        }
    } else if (ok) {
        for (int t = g; t < Tp; t += 4) {
            float u, du;
            load(t, u, du);
            p1 += du; p2 += mul_rounded(du, u);
        }
    }
    s1[g][cl] = p1; s2[g][cl] = p2;
    __syncthreads();
    const float m1 = (s1[0][cl] + s1[1][cl] + s1[2][cl] + s1[3][cl]) / (float)Tp;
    const float m2 = (s2[0][cl] + s2[1][cl] + s2[2][cl] + s2[3][cl]) / (float)Tp;
    const float rs = ok ? rstd[(size_t)b * C + c] : 0.f;
    if (R > 0) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int t = g + 4 * i;
            if (ok && t < Tp) d[(size_t)t * C] = rs * (dd[i] - m1 - uu[i] * m2);
        }
    } else if (ok) {
        for (int t = g; t < Tp; t += 4) {
            float u, du;
            load(t, u, du);
            d[(size_t)t * C] = rs * fmaf(-u, m2, du - m1);
        }
    }
}

// the instantiation a launch takes: the policy from L.norm / L.act, the form from the batch's longest clip (the register
// forms are InstanceNorm's alone), the rule from the rows
template <int NORM, int ACT, int R, int RULE>
static void norm_act_go(const NormActLaunch& L, bool backward, hipStream_t st) {
    const dim3 grid((L.C + 63) / 64, L.B), block(256);
    if (backward)
        hipLaunchKernelGGL((norm_act_bwd_kernel<NORM, ACT, R, RULE>), grid, block, 0, st, L.x, L.out, L.stash, L.frame_off,
                           L.pool_off, L.rstd, L.scale, L.C, L.rows);
    else
        hipLaunchKernelGGL((norm_act_fwd_kernel<NORM, ACT, R, RULE>), grid, block, 0, st, L.x, L.frame_off, L.pool_off, L.rstd,
                           L.scale, L.shift, L.stash, L.C, L.rows);
}
template <int NORM, int ACT, int R>
static void norm_act_rows(const NormActLaunch& L, bool backward, hipStream_t st) {
    switch (rows_rule(L.rows)) {
        case kRowsPool: norm_act_go<NORM, ACT, R, kRowsPool>(L, backward, st); break;
        case kRowsTaps: norm_act_go<NORM, ACT, R, kRowsTaps>(L, backward, st); break;
        default: norm_act_go<NORM, ACT, R, kRowsHalf>(L, backward, st);
    }
}
template <int NORM, int ACT>
static void norm_act_form(const NormActLaunch& L, bool backward, hipStream_t st) {
    if constexpr (NORM == kNormInstance) {
        if (L.max_pooled <= 128) return norm_act_rows<NORM, ACT, 32>(L, backward, st);
        if (L.max_pooled <= 320) return norm_act_rows<NORM, ACT, 80>(L, backward, st);
    }
    norm_act_rows<NORM, ACT, 0>(L, backward, st);
}
template <int NORM>
static void norm_act_policy(const NormActLaunch& L, bool backward, hipStream_t st) {
    switch (L.act) {
        case kActRelu: norm_act_form<NORM, kActRelu>(L, backward, st); break;
        case kActLRelu: norm_act_form<NORM, kActLRelu>(L, backward, st); break;
        case kActGelu: norm_act_form<NORM, kActGelu>(L, backward, st); break;
        default: norm_act_form<NORM, kActSwish>(L, backward, st); break;
    }
}
void launch_norm_act(const NormActLaunch& L, bool backward, hipStream_t st) {
    if (L.norm == kNormInstance) norm_act_policy<kNormInstance>(L, backward, st);
    else if (L.norm == kNormAffine) norm_act_policy<kNormAffine>(L, backward, st);
    else norm_act_policy<kNormNone>(L, backward, st);
}

// ---------------------------------------------------------------------------------
// BRH read-out + loss + gradient seed.  One 64-thread workgroup per clip.
// loss_kind: 0 push_extremes, 1 mse, 2 hinge, 3 sign, 4 push_sigmoid, 5 ber  (embedding/losses.py)
// FA: the final activation (act_fwd / act_grad; the model card's tanh is written out as it always was).
// If dA3 == nullptr only the prediction is produced (detect path).
// ---------------------------------------------------------------------------------
template <int FA, bool POOL>
__global__ __launch_bounds__(256) void head_kernel(const float* __restrict__ a3, const int* __restrict__ frame_off, const int* __restrict__ pool_off,
                                                    const float* __restrict__ target, float* __restrict__ pred,
                                                    float* __restrict__ loss_out, float* __restrict__ best_loss,
                                                    int* __restrict__ improved, float* __restrict__ dA3, int* __restrict__ step,
                                                    int loss_kind, int nbits, const float* __restrict__ loss_add, int C,
                                                    TapRows rows) {
    // C: channel pitch of a3 / dA3, 2 * nbits or the detector's padded count (channels 2 * nbits .. C-1 are never read out;
    // their dA3 is zero)
    __shared__ float part[4][64], mean[64], dm[64];
    const int b = blockIdx.x, c = threadIdx.x & 63, g = threadIdx.x >> 6;
    // rows are 32-aligned per clip (POOL: an initial pool other than (2, 2))
    const int r0 = pool_off[b], Tp = rows.of(rows_l0<POOL ? kRowsPool : kRowsHalf>(frame_off[b + 1] - frame_off[b], rows));
    float m = 0.f;
    if (c < C)
        for (int t = g; t < Tp; t += 4) m += a3[(size_t)(r0 + t) * C + c];
    part[g][c] = m;
    __syncthreads();
    if (g == 0) mean[c] = (part[0][c] + part[1][c] + part[2][c] + part[3][c]) / (float)Tp;
    __syncthreads();
    float lterm = 0.f, dp = 0.f, p = 0.f, xd = 0.f;
    if (g == 0 && c < nbits) {
        xd = mean[2 * c] - mean[2 * c + 1];
        p = FA == kActTanh ? tanhf(xd) : act_fwd<FA>(xd);
        pred[b * nbits + c] = p;
        if (target) {
            const float tg = target[b * nbits + c];
            const float inv = 1.0f / (float)nbits;
            loss_term(loss_kind, p, tg, inv, lterm, dp);
        }
    }
    if (!target) return;
    if (g == 0) {
        float L = wave_sum(lterm);
        if (loss_add) L += loss_add[b];                          // per-clip term computed elsewhere (L1 on the coefficients)
        if (c == 0) {
            loss_out[b] = L;
            if (best_loss) {                                     // null: gradient-only call, no bookkeeping
                const float bl = best_loss[b];
                const int imp = L < bl;
                improved[b] = imp;
                if (imp) best_loss[b] = L;
            }
            if (step && b == 0) *step += 1;
        }
        if (dA3 && c < nbits) {
            const float dpre = dp * (FA == kActTanh ? 1.f - p * p : act_grad<FA>(xd, p));   // tanh' on the card
            dm[2 * c] = dpre; dm[2 * c + 1] = -dpre;
        }
    }
    if (!dA3) return;
    __syncthreads();
    if (c < C) {
        const float gv = c < 2 * nbits ? dm[c] / (float)Tp : 0.f;
        for (int t = g; t < Tp; t += 4) dA3[(size_t)(r0 + t) * C + c] = gv;
    }
}

// ---------------------------------------------------------------------------------
// Fused tail of the detector for clips of up to 4*R pooled frames (R = 32, or 80 for clips up to 10 s): sum of the last conv's
// split-K partials + bias -> InstanceNorm -> LeakyReLU -> BRH read-out -> loss / best-loss
// bookkeeping -> gradient back through the read-out, LeakyReLU and InstanceNorm.
// One 256-thread workgroup per clip (64 channel slots x 4 row groups, activation in registers).
// Writes pred, loss, improved, best_loss and dZ = dL/d(conv output) [rows][C]; advances the
// optimiser step counter (block 0) when step != nullptr.
// ---------------------------------------------------------------------------------
template <int NSPLIT, int R>
__global__ __launch_bounds__(256) void tail_kernel(const float* __restrict__ zpart, size_t slab,
                                                    const float* __restrict__ bias, const int* __restrict__ frame_off,
                                                    const int* __restrict__ pool_off, const float* __restrict__ target,
                                                    float* __restrict__ pred, float* __restrict__ loss_out,
                                                    float* __restrict__ best_loss, int* __restrict__ improved,
                                                    float* __restrict__ dZ, int* __restrict__ step, int loss_kind, int nbits,
                                                    const float* __restrict__ loss_add, int ldz, int C) {
    // C: channel pitch of zpart, 2 * nbits or the detector's padded count (padding channels: zero weights and bias, never
    // read out, dZ zero).  ldz: row pitch of dZ, C or 64 (columns C..63 are then written as zeros: K padding of the
    // data-gradient GEMM)
    __shared__ float red[4][64], red2[4][64], mean_s[64], dm[64];
    const int b = blockIdx.x, c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int r0 = pool_off[b], Tp = (frame_off[b + 1] - frame_off[b]) / 2;
    const bool ok = c < C;
    const float invT = 1.0f / (float)Tp;
    float z[R];
    const float bv = (ok && bias) ? bias[c] : 0.f;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int t = g + 4 * i;
        // clamped index + mask instead of a branch around the loads (they would wait one by one)
        const int tc = t < Tp ? t : Tp - 1;
        const int cc = ok ? c : C - 1;
        float part[NSPLIT];
#pragma unroll
        for (int k = 0; k < NSPLIT; ++k) part[k] = zpart[k * slab + (size_t)(r0 + tc) * C + cc];
        float acc = bv;
#pragma unroll
        for (int k = 0; k < NSPLIT; ++k) acc += part[k];
        z[i] = (ok && t < Tp) ? acc : 0.f;
        s += z[i];
    }
    red[g][c] = s;
    __syncthreads();
    const float mu = (red[0][c] + red[1][c] + red[2][c] + red[3][c]) * invT;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < R; ++i)
        if (g + 4 * i < Tp) { const float d = z[i] - mu; q += d * d; }
    red2[g][c] = q;
    __syncthreads();
    const float rs = 1.0f / sqrtf((red2[0][c] + red2[1][c] + red2[2][c] + red2[3][c]) * invT + 1e-5f);
    // u = normalised pre-activation (kept in z), read-out mean of LeakyReLU(u)
    float am = 0.f;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const float u = (z[i] - mu) * rs;
        z[i] = u;
        if (g + 4 * i < Tp) am += (u > 0.f ? u : 0.2f * u);
    }
    __syncthreads();
    red[g][c] = am;
    __syncthreads();
    if (g == 0) mean_s[c] = ok ? (red[0][c] + red[1][c] + red[2][c] + red[3][c]) * invT : 0.f;
    __syncthreads();
    float lterm = 0.f, dp = 0.f, p = 0.f;
    if (g == 0 && c < nbits) {
        p = tanhf(mean_s[2 * c] - mean_s[2 * c + 1]);
        pred[b * nbits + c] = p;
        if (target) {
            const float tg = target[b * nbits + c];
            const float inv = 1.0f / (float)nbits;
            loss_term(loss_kind, p, tg, inv, lterm, dp);
        }
    }
    if (!target) return;
    if (g == 0) {
        float L = wave_sum(lterm);
        if (loss_add) L += loss_add[b];                          // per-clip term computed elsewhere (L1 on the coefficients)
        if (c == 0) {
            loss_out[b] = L;
            if (best_loss) {                                     // null: gradient-only call, no bookkeeping
                const float bl = best_loss[b];
                const int imp = L < bl;
                improved[b] = imp;
                if (imp) best_loss[b] = L;
            }
            if (step && b == 0) *step += 1;
        }
        if (c < nbits) {
            const float dpre = dp * (1.f - p * p);             // tanh'
            dm[2 * c] = dpre; dm[2 * c + 1] = -dpre;
        }
    }
    if (!dZ) return;
    __syncthreads();
    // dA[t][c] = dm[c]/Tp ; dU = dA * lrelu'(u) ; InstanceNorm backward
    const float ga = c < 2 * nbits ? dm[c] * invT : 0.f;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < R; ++i)
        if (g + 4 * i < Tp) { const float du = ga * (z[i] > 0.f ? 1.f : 0.2f); s1 += du; s2 += du * z[i]; }
    red[g][c] = s1; red2[g][c] = s2;
    __syncthreads();
    const float m1 = (red[0][c] + red[1][c] + red[2][c] + red[3][c]) * invT;
    const float m2 = (red2[0][c] + red2[1][c] + red2[2][c] + red2[3][c]) * invT;
    const int Tpad = (Tp + 31) & ~31;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int t = g + 4 * i;
        if (c < ldz && t < Tpad) {
            const float du = ga * (z[i] > 0.f ? 1.f : 0.2f);
            dZ[(size_t)(r0 + t) * ldz + c] = (ok && t < Tp) ? rs * (du - m1 - z[i] * m2) : 0.f;
        }
    }
}

void launch_tail(const float* zpart, int nsplit, size_t slab, const float* bias, const int* frame_off, const int* pool_off,
                 const float* target, float* pred, float* loss, float* best_loss, int* improved, float* dZ, int* step,
                 int loss_kind, int nbits, int B, int max_pooled, hipStream_t st, const float* loss_add, int ldz, int C) {
    if (C < 2 * nbits) C = 2 * nbits;
    if (ldz < C) ldz = C;
#define TL(S_, R_) hipLaunchKernelGGL((tail_kernel<S_, R_>), dim3(B), dim3(256), 0, st, zpart, slab, bias, frame_off, pool_off, \
                                      target, pred, loss, best_loss, improved, dZ, step, loss_kind, nbits, loss_add, ldz, C)
    if (max_pooled <= 128) { if (nsplit == 4) TL(4, 32); else TL(1, 32); }
    else { if (nsplit == 4) TL(4, 80); else TL(1, 80); }
#undef TL
}
// ---------------------------------------------------------------------------------
// Wide BRH read-out for detectors whose last block has 64 < C <= 1024 channels (payloads of 33 .. 512 bits; the block is
// stored with Cp = C rounded up to a multiple of 128, padding channels all zero).  One 256-thread workgroup per clip; it
// walks the clip's pooled frames in a loop, so any clip length is served with a fixed register budget.  Thread = channel
// slot cl of CW = min(Cp, 256) and time group g of 256 / CW; it owns channels cl, cl + CW, ... (at most kWideNJ).
//   pass 1: per-channel time sums of the block output A (card: also of lrelu'(u) and lrelu'(u) u, u recovered from A)
//   read-out: mean -> even - odd -> final activation -> loss / best-loss bookkeeping / step counter, as head_kernel
//   pass 2: MODE 1: dL/dA [rows][Cp] (staged route: the backward of launch_norm_act consumes it)
//           MODE 2: dL/dZ of the card block, the InstanceNorm + LeakyReLU backward folded in (dA is constant in time, so
//                   mean_t dU = dA mean_t lrelu' and mean_t dU u = dA mean_t lrelu' u come from pass 1), and the per-clip
//                   partial maxima of |dZ| for the f16 two-term data-gradient GEMM (gmax [B][64]: entry 0 the maximum,
//                   entries 1 .. Cp/16 - 1 zero), when gmax is given
// Rows Tp .. Tp rounded up to 32 (the clip's padding rows) and padding channels get a zero gradient.  MODE 0: pred only.
// ---------------------------------------------------------------------------------
constexpr int kWideNJ = 4;
constexpr int kWideMaxC = 1024;
template <int FA, int MODE, bool POOL>
__global__ __launch_bounds__(256) void readout_wide_kernel(const float* __restrict__ A, int Cp, const int* __restrict__ frame_off,
                                                            const int* __restrict__ pool_off, const float* __restrict__ rstd,
                                                            const float* __restrict__ target, float* __restrict__ pred,
                                                            float* __restrict__ loss_out, float* __restrict__ best_loss,
                                                            int* __restrict__ improved, float* __restrict__ dout,
                                                            float* __restrict__ gmax, int* __restrict__ step, int loss_kind,
                                                            int nbits, const float* __restrict__ loss_add, TapRows rows) {
    __shared__ float s_a[kWideMaxC], s_l[kWideMaxC], s_lu[kWideMaxC];
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int CW = Cp < 256 ? Cp : 256, NG = 256 / CW;
    const int cl = tid % CW, g = tid / CW;
    // rows are 32-aligned per clip (POOL: an initial pool other than (2, 2))
    const int r0 = pool_off[b], Tp = rows.of(rows_l0<POOL ? kRowsPool : kRowsHalf>(frame_off[b + 1] - frame_off[b], rows));
    const int C = 2 * nbits;
    const float invT = 1.0f / (float)Tp;
    float sa[kWideNJ], sl[kWideNJ], slu[kWideNJ];
#pragma unroll
    for (int j = 0; j < kWideNJ; ++j) { sa[j] = 0.f; sl[j] = 0.f; slu[j] = 0.f; }
    for (int t = g; t < Tp; t += NG) {
        const float* row = A + (size_t)(r0 + t) * Cp;
#pragma unroll
        for (int j = 0; j < kWideNJ; ++j) {
            const int c = cl + CW * j;
            if (c < Cp) {
                const float a = row[c];
                sa[j] += a;
                if (MODE == 2) {
                    const float sg = a > 0.f ? 1.f : 0.2f;
                    sl[j] += sg;
                    slu[j] += sg * (a > 0.f ? a : a * 5.0f);   // lrelu'(u) u, u = LeakyReLU(0.2)^-1 (a)
                }
            }
        }
    }
    // time groups -> per-channel sums in LDS (g = 0 writes, the others add in order)
    for (int gg = 0; gg < NG; ++gg) {
        if (g == gg) {
#pragma unroll
            for (int j = 0; j < kWideNJ; ++j) {
                const int c = cl + CW * j;
                if (c < Cp) {
                    s_a[c] = gg ? s_a[c] + sa[j] : sa[j];
                    if (MODE == 2) { s_l[c] = gg ? s_l[c] + sl[j] : sl[j]; s_lu[c] = gg ? s_lu[c] + slu[j] : slu[j]; }
                }
            }
        }
        __syncthreads();
    }
    // read-out and loss; dmv = dL/d(even - odd) of the bits this thread owns
    float lterm = 0.f;
    float dmv[(kWideMaxC / 2 + 255) / 256];
#pragma unroll
    for (int i = 0; i < (kWideMaxC / 2 + 255) / 256; ++i) {
        const int k = tid + 256 * i;
        dmv[i] = 0.f;
        if (k < nbits) {
            const float xd = s_a[2 * k] * invT - s_a[2 * k + 1] * invT;
            const float p = FA == kActTanh ? tanhf(xd) : act_fwd<FA>(xd);
            pred[(size_t)b * nbits + k] = p;
            if (MODE != 0) {
                const float tg = target[(size_t)b * nbits + k];
                float lt = 0.f, dp = 0.f;
                loss_term(loss_kind, p, tg, 1.0f / (float)nbits, lt, dp);
                lterm += lt;
                dmv[i] = dp * (FA == kActTanh ? 1.f - p * p : act_grad<FA>(xd, p));
            }
        }
    }
    if (MODE == 0) return;
    float Ls = block_sum(lterm, red);
    if (tid == 0) {
        if (loss_add) Ls += loss_add[b];                          // per-clip term computed elsewhere (L1 on the coefficients)
        loss_out[b] = Ls;
        if (best_loss) {                                          // null: gradient-only call, no bookkeeping
            const float bl = best_loss[b];
            const int imp = Ls < bl;
            improved[b] = imp;
            if (imp) best_loss[b] = Ls;
        }
        if (step && b == 0) *step += 1;
    }
    if (!dout) return;
    // s_a is free from here on: it takes dL/dA = dm / Tp per channel (zero for padding channels)
    __syncthreads();
#pragma unroll
    for (int i = 0; i < (kWideMaxC / 2 + 255) / 256; ++i) {
        const int k = tid + 256 * i;
        if (k < nbits) { s_a[2 * k] = dmv[i] * invT; s_a[2 * k + 1] = -dmv[i] * invT; }
    }
    for (int c = C + tid; c < Cp; c += 256) s_a[c] = 0.f;
    __syncthreads();
    float ga[kWideNJ], m1[kWideNJ], m2[kWideNJ], rs[kWideNJ];
#pragma unroll
    for (int j = 0; j < kWideNJ; ++j) {
        const int c = cl + CW * j;
        const bool ok = c < Cp;
        ga[j] = ok ? s_a[c] : 0.f;
        m1[j] = MODE == 2 && ok ? ga[j] * (s_l[c] * invT) : 0.f;
        m2[j] = MODE == 2 && ok ? ga[j] * (s_lu[c] * invT) : 0.f;
        rs[j] = MODE == 2 && ok ? rstd[(size_t)b * Cp + c] : 0.f;
    }
    const int Tpad = (Tp + 31) & ~31;
    float mx = 0.f;
    for (int t = g; t < Tpad; t += NG) {
        const float* row = A + (size_t)(r0 + t) * Cp;
        float* drow = dout + (size_t)(r0 + t) * Cp;
#pragma unroll
        for (int j = 0; j < kWideNJ; ++j) {
            const int c = cl + CW * j;
            if (c < Cp) {
                float v = 0.f;
                if (t < Tp) {
                    if (MODE == 2) {
                        const float a = row[c];
                        const float u = a > 0.f ? a : a * 5.0f;
                        const float du = ga[j] * (a > 0.f ? 1.f : 0.2f);
                        v = rs[j] * (du - m1[j] - u * m2[j]);
                        mx = fmaxf(mx, fabsf(v));
                    } else {
                        v = ga[j];
                    }
                }
                drow[c] = v;
            }
        }
    }
    if (MODE == 2 && gmax) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = mx;
        __syncthreads();
        if (tid < Cp / 16) gmax[(size_t)b * 64 + tid] = tid == 0 ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : 0.f;
    }
}

void launch_readout_wide(const float* A, int Cp, const int* frame_off, const int* pool_off, const float* rstd, const float* target,
                         float* pred, float* loss, float* best_loss, int* improved, float* dout, float* gmax, int* step,
                         int loss_kind, int nbits, int B, hipStream_t st, const float* loss_add, int final_act, bool card_bwd,
                         TapRows rows) {
    const int mode = !target ? 0 : (card_bwd ? 2 : 1);
    // (a detector with an initial pool other than (2, 2) is never the card's: its instantiations are modes 0 and 1 alone)
    const bool pool = rows.pooled();
#define AW_WIDE(FA, M, P)                                                                                                    \
    hipLaunchKernelGGL((readout_wide_kernel<FA, M, P>), dim3(B), dim3(256), 0, st, A, Cp, frame_off, pool_off, rstd, target, pred, \
                       loss, best_loss, improved, dout, gmax, step, loss_kind, nbits, loss_add, rows)
#define AW_WIDE_FA(FA)                                                                     \
    do {                                                                                   \
        if (pool) { if (mode == 0) AW_WIDE(FA, 0, true); else AW_WIDE(FA, 1, true); }      \
        else if (mode == 0) AW_WIDE(FA, 0, false);                                         \
        else if (mode == 1) AW_WIDE(FA, 1, false);                                         \
        else AW_WIDE(FA, 2, false);                                                        \
    } while (0)
    switch (final_act) {
        case kActRelu: AW_WIDE_FA(kActRelu); break;
        case kActLRelu: AW_WIDE_FA(kActLRelu); break;
        case kActGelu: AW_WIDE_FA(kActGelu); break;
        case kActSwish: AW_WIDE_FA(kActSwish); break;
        case kActSigmoid: AW_WIDE_FA(kActSigmoid); break;
        default: AW_WIDE_FA(kActTanh); break;
    }
#undef AW_WIDE_FA
#undef AW_WIDE
}
// ---------------------------------------------------------------------------------
// The same mel block for clips of at most 192 frames in ONE launch per direction: one 512-thread workgroup per clip
// keeps the clip's [T][128] tile in registers (thread = channel c, pooled rows g, g+4, ...: the frame pair
// (2tp, 2tp+1)), so the statistics need no second pass over memory and no partial buffers.
// ---------------------------------------------------------------------------------
constexpr int kMelClipR = kMelClipFrames / 8;       // frame pairs per thread

// sum over the 4 row groups of a channel (threads c, c+128, c+256, c+384), result for every thread
__device__ __forceinline__ float mel_chan_sum(float v, float (*red)[128], int c, int g) {
    __syncthreads();
    red[g][c] = v;
    __syncthreads();
    return (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

// amax_out: [B][64] partial maxima of |x0| per clip (entries 0..7 written: the maximum, then zeros) for gemm_h2.hip, or null
__global__ __launch_bounds__(512) void mel_norm_clip_fwd_kernel(const float* __restrict__ xm, const int* __restrict__ frame_off,
                                                                 const int* __restrict__ pool_off, float* __restrict__ x0,
                                                                 float* __restrict__ stats, float* __restrict__ gstat,
                                                                 float* __restrict__ amax_out) {
    __shared__ float red[4][128];
    __shared__ float red8[8];
    const int b = blockIdx.x;
    const int f0 = frame_off[b], T = frame_off[b + 1] - f0, Tp = T / 2;
    const int c = threadIdx.x & 127, g = threadIdx.x >> 7;
    const float* x = xm + (size_t)f0 * 128 + c;
    float xa[kMelClipR], xb[kMelClipR];
#pragma unroll
    for (int i = 0; i < kMelClipR; ++i) {                   // loads first, from clamped rows; masked below
        const int t = 2 * (g + 4 * i);
        xa[i] = x[(size_t)min(t, T - 1) * 128];
        xb[i] = x[(size_t)min(t + 1, T - 1) * 128];
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kMelClipR; ++i) {
        const int t = 2 * (g + 4 * i);
        if (t < T) s += xa[i];
        if (t + 1 < T) s += xb[i];
    }
    const float mu = mel_chan_sum(s, red, c, g) / (float)T;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < kMelClipR; ++i) {
        const int t = 2 * (g + 4 * i);
        if (t < T) { const float d = xa[i] - mu; q += d * d; }
        if (t + 1 < T) { const float d = xb[i] - mu; q += d * d; }
    }
    const float M2 = mel_chan_sum(q, red, c, g);
    const float rs = mel_rs(M2, (float)T);
    const float suu = mel_block_sum(g == 0 ? mel_suu(rs, M2) : 0.f, red8);
    const MelClip k = mel_clip(suu, (float)T, 128);
    if (g == 0) mel_write_stats(stats, (size_t)b * 128 + c, mu, rs, M2);
    if (threadIdx.x == 0) mel_write_gstat(gstat, b, k, (float)T);
    float* o = x0 + (size_t)pool_off[b] * 128 + c;
    const int Tpad = (Tp + 31) & ~31;
    float omax = 0.f;
#pragma unroll
    for (int i = 0; i < kMelClipR; ++i) {
        const int tp = g + 4 * i;
        const float u0 = mel_u(xa[i], mu, rs), u1 = mel_u(xb[i], mu, rs);
        if (tp < Tp) {
            const float v = mel_pooled(u0, u1, k.ginv);
            o[(size_t)tp * 128] = v;
            omax = fmaxf(omax, fabsf(v));
        } else if (tp < Tpad) o[(size_t)tp * 128] = 0.f;                          // pad rows stay finite
    }
    if (amax_out) {
#pragma unroll
        for (int of = 32; of > 0; of >>= 1) omax = fmaxf(omax, __shfl_xor(omax, of));
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red8[threadIdx.x >> 6] = omax;
        __syncthreads();
        if (threadIdx.x < 8) {
            float m = red8[0];
#pragma unroll
            for (int w = 1; w < 8; ++w) m = fmaxf(m, red8[w]);
            amax_out[(size_t)b * 64 + threadIdx.x] = threadIdx.x == 0 ? m : 0.f;
        }
    }
}

__global__ __launch_bounds__(512) void mel_norm_clip_bwd_kernel(const float* __restrict__ dx0, float* __restrict__ xm,
                                                                 const int* __restrict__ frame_off, const int* __restrict__ pool_off,
                                                                 const float* __restrict__ stats, const float* __restrict__ gstat) {
    __shared__ float red[4][128];
    __shared__ float red8[8];
    const int b = blockIdx.x;
    const int f0 = frame_off[b], T = frame_off[b + 1] - f0, Tp = T / 2;
    const int c = threadIdx.x & 127, g = threadIdx.x >> 7;
    const MelChan s = mel_read_stats(stats, (size_t)b * 128 + c);
    const MelClip k = mel_read_gstat(gstat, b);
    float* x = xm + (size_t)f0 * 128 + c;
    const float* d0 = dx0 + (size_t)pool_off[b] * 128 + c;
    float xa[kMelClipR], xb[kMelClipR], dd[kMelClipR];
#pragma unroll
    for (int i = 0; i < kMelClipR; ++i) {
        const int tp = g + 4 * i, t = 2 * tp;
        xa[i] = x[(size_t)min(t, T - 1) * 128];
        xb[i] = x[(size_t)min(t + 1, T - 1) * 128];
        dd[i] = d0[(size_t)min(tp, max(Tp - 1, 0)) * 128];
    }
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int i = 0; i < kMelClipR; ++i) {
        const bool pair = g + 4 * i < Tp;
        const float dv = pair ? 0.5f * dd[i] : 0.f;                   // d(avg pool): half the pooled gradient to each frame
        dd[i] = dv;
        xa[i] = mel_u(xa[i], s.mu, s.rs);
        xb[i] = mel_u(xb[i], s.mu, s.rs);
        if (pair) { a1 += 2.f * dv; a2 += mel_dv_u(dv, xa[i], xb[i]); }
    }
    const float D1 = mel_chan_sum(a1, red, c, g), D2 = mel_chan_sum(a2, red, c, g);
    const float sa = mel_block_sum(g == 0 ? D1 : 0.f, red8);
    const float sb = mel_block_sum(g == 0 ? D2 : 0.f, red8);
    const MelClipGrad q = mel_clip_grad(sa, sb, k);
    const MelChanGrad m = mel_chan_grad(D1, D2, (float)T, s.rs, s.M2, k, q);
#pragma unroll
    for (int i = 0; i < kMelClipR; ++i) {
        const int t = 2 * (g + 4 * i);
        if (t < T) x[(size_t)t * 128] = mel_bwd_value(dd[i], xa[i], s.rs, k.ginv, q, m);
        if (t + 1 < T) x[(size_t)(t + 1) * 128] = mel_bwd_value(dd[i], xb[i], s.rs, k.ginv, q, m);
    }
}

// ---------------------------------------------------------------------------------
// The clip form for any bank (MelBankAny's layout above): one 512-thread workgroup per clip, 4 row groups; each 128-channel
// group's statistics are complete before the next starts, and the passes over the clip's rows -- mean, M2, output -- re-read
// it from L2 (frames g, g + 4, ...), where the 128-band kernels above sum frame pairs held in registers: another order of the
// same sums, so the two stay apart.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void mel_any_clip_fwd_kernel(const float* __restrict__ xm, const int* __restrict__ frame_off,
                                                                const int* __restrict__ pool_off, float* __restrict__ x0,
                                                                float* __restrict__ stats, float* __restrict__ gstat, int n_mels,
                                                                int Mp) {
    __shared__ float red[4][128];
    __shared__ float red8[8];
    __shared__ float smu[MelBankAny::kGroups][128], srs[MelBankAny::kGroups][128];   // the statistics of the output pass
    const int b = blockIdx.x;
    const int f0 = frame_off[b], T = frame_off[b + 1] - f0, Tp = T / 2;
    const int c = threadIdx.x & 127, g = threadIdx.x >> 7;
    const int ng = (Mp + 127) / 128;
    float suu = 0.f;
#pragma unroll 1
    for (int j = 0; j < ng; ++j) {                                     // ng is uniform across the workgroup
        const int ch = 128 * j + c;
        const bool on = ch < n_mels;
        // row group g takes frames g, g + 4, ...: two passes over the clip's column (mean, then M2); the clip stays in L2
        const float* x = xm + (size_t)f0 * Mp + min(ch, n_mels - 1);
        float sm = 0.f;
        for (int t = g; t < T; t += 4) sm += x[(size_t)t * Mp];
        const float mu = mel_chan_sum(sm, red, c, g) / (float)T;
        float q = 0.f;
        for (int t = g; t < T; t += 4) { const float d = x[(size_t)t * Mp] - mu; q += d * d; }
        const float M2 = mel_chan_sum(q, red, c, g);
        const float rs = mel_rs(M2, (float)T);
        if (g == 0 && ch < Mp) mel_write_stats(stats, (size_t)b * Mp + ch, on ? mu : 0.f, on ? rs : 0.f, on ? M2 : 0.f);
        if (on && g == 0) suu += mel_suu(rs, M2);
        if (g == 0) { smu[j][c] = on ? mu : 0.f; srs[j][c] = on ? rs : 0.f; }
    }
    suu = mel_block_sum(suu, red8);
    const MelClip k = mel_clip(suu, (float)T, n_mels);
    if (threadIdx.x == 0) mel_write_gstat(gstat, b, k, (float)T);
    const int Tpad = (Tp + 31) & ~31;
#pragma unroll 1
    for (int j = 0; j < ng; ++j) {
        const int ch = 128 * j + c;
        if (ch >= Mp) continue;
        const float* x = xm + (size_t)f0 * Mp + ch;
        float* o = x0 + (size_t)pool_off[b] * Mp + ch;
        const float mu = smu[j][c], rs = srs[j][c];
        for (int tp = g; tp < Tpad; tp += 4) {
            float v = 0.f;                                            // pad rows and padding channels stay zero
            if (tp < Tp && ch < n_mels)
                v = mel_pooled(mel_u(x[(size_t)(2 * tp) * Mp], mu, rs), mel_u(x[(size_t)(2 * tp + 1) * Mp], mu, rs), k.ginv);
            o[(size_t)tp * Mp] = v;
        }
    }
}

__global__ __launch_bounds__(512) void mel_any_clip_bwd_kernel(const float* __restrict__ dx0, float* __restrict__ xm,
                                                                const int* __restrict__ frame_off, const int* __restrict__ pool_off,
                                                                const float* __restrict__ stats, const float* __restrict__ gstat,
                                                                int n_mels, int Mp) {
    constexpr int kGroups = MelBankAny::kGroups;
    __shared__ float red[4][128];
    __shared__ float red8[8];
    const int b = blockIdx.x;
    const int f0 = frame_off[b], T = frame_off[b + 1] - f0, Tp = T / 2;
    const int c = threadIdx.x & 127, g = threadIdx.x >> 7;
    const int ng = (Mp + 127) / 128;
    const MelClip k = mel_read_gstat(gstat, b);
    float d1s[kGroups], d2s[kGroups];
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int j = 0; j < kGroups; ++j) {
        d1s[j] = 0.f; d2s[j] = 0.f;
        if (j >= ng) continue;                                         // uniform across the workgroup
        const int ch = 128 * j + c;
        const bool on = ch < n_mels;
        const int cc = min(ch, n_mels - 1);
        const MelChan s = mel_read_stats(stats, (size_t)b * Mp + cc);
        const float* x = xm + (size_t)f0 * Mp + cc;
        const float* d0 = dx0 + (size_t)pool_off[b] * Mp + cc;
        float a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int i = 0; i < kMelClipR; ++i) {
            const int tp = g + 4 * i, t = 2 * tp;
            if (tp < Tp) {
                const float dv = 0.5f * d0[(size_t)tp * Mp];           // d(avg pool): half the pooled gradient to each frame
                const float u0 = mel_u(x[(size_t)t * Mp], s.mu, s.rs), u1 = mel_u(x[(size_t)(t + 1) * Mp], s.mu, s.rs);
                a1 += 2.f * dv;
                a2 += mel_dv_u(dv, u0, u1);
            }
        }
        const float D1 = mel_chan_sum(a1, red, c, g), D2 = mel_chan_sum(a2, red, c, g);
        if (on && g == 0) { sa += D1; sb += D2; }
        d1s[j] = D1; d2s[j] = D2;
    }
    sa = mel_block_sum(sa, red8);
    sb = mel_block_sum(sb, red8);
    const MelClipGrad q = mel_clip_grad(sa, sb, k);
    // every read of the clip's xm above is complete (the block sums hold barriers): the in-place writes start here
#pragma unroll
    for (int j = 0; j < kGroups; ++j) {
        const int ch = 128 * j + c;
        if (j >= ng || ch >= Mp) continue;
        float* x = xm + (size_t)f0 * Mp + ch;
        if (ch >= n_mels) {
            for (int t = g; t < T; t += 4) x[(size_t)t * Mp] = 0.f;
            continue;
        }
        const MelChan s = mel_read_stats(stats, (size_t)b * Mp + ch);
        const float* d0 = dx0 + (size_t)pool_off[b] * Mp + ch;
        const MelChanGrad m = mel_chan_grad(d1s[j], d2s[j], (float)T, s.rs, s.M2, k, q);
        for (int t = g; t < T; t += 4) {
            const float dv = (t < 2 * Tp) ? 0.5f * d0[(size_t)(t >> 1) * Mp] : 0.f;
            x[(size_t)t * Mp] = mel_bwd_value(dv, mel_u(x[(size_t)t * Mp], s.mu, s.rs), s.rs, k.ginv, q, m);
        }
    }
}

// The chunked form's two launches per direction, for one bank: a block per 32-frame chunk and clip.
template <class Bank>
static void mel_chunked_fwd(const float* xm, const int* frame_off, const int* pool_off, float* x0, float* stats, float* gstat,
                            float* part, int pstride, int B, int max_frames, int n_mels, int Mp, hipStream_t st) {
    const dim3 grid((max_frames + kMelChunk - 1) / kMelChunk, B);
    hipLaunchKernelGGL(mel_partial_stats_kernel<Bank>, grid, dim3(256), 0, st, xm, frame_off, part, pstride, n_mels, Mp);
    hipLaunchKernelGGL(mel_apply_pool_kernel<Bank>, grid, dim3(256), 0, st, xm, frame_off, pool_off, part, pstride, x0, stats,
                       gstat, n_mels, Mp);
}
template <class Bank>
static void mel_chunked_bwd(const float* dx0, float* xm, const int* frame_off, const int* pool_off, const float* stats,
                            const float* gstat, float* part, int pstride, int B, int max_frames, int n_mels, int Mp,
                            hipStream_t st) {
    const dim3 grid((max_frames + kMelChunk - 1) / kMelChunk, B);
    hipLaunchKernelGGL(mel_bwd_partial_kernel<Bank>, grid, dim3(256), 0, st, dx0, xm, frame_off, pool_off, stats, part, pstride,
                       n_mels, Mp);
    hipLaunchKernelGGL(mel_bwd_apply_kernel<Bank>, grid, dim3(256), 0, st, dx0, xm, frame_off, pool_off, stats, gstat, part,
                       pstride, n_mels, Mp);
}

// the chunked form's first launch on its own, for the pooled nets' kernels (mel_pool_kernels.hip), which share it
void launch_mel_partial_stats(const float* xm, const int* frame_off, float* part, int pstride, int B, int max_frames, int n_mels,
                              int Mp, hipStream_t st) {
    const dim3 grid((max_frames + kMelChunk - 1) / kMelChunk, B);
    if (n_mels == 128)
        hipLaunchKernelGGL(mel_partial_stats_kernel<MelBank128>, grid, dim3(256), 0, st, xm, frame_off, part, pstride, n_mels, Mp);
    else
        hipLaunchKernelGGL(mel_partial_stats_kernel<MelBankAny>, grid, dim3(256), 0, st, xm, frame_off, part, pstride, n_mels, Mp);
}

// One launcher per direction: the clip form up to kMelClipFrames frames, else the chunked two-launch form; the 128-band
// instantiations for the card's bank, else the any-bank ones.  n_mels <= 512 bands in rows of Mp >= n_mels floats
// (Mp % 4 == 0); stats [B][Mp][4], part [B][pstride][2 Mp].
void launch_mel_norm_fwd(const float* xm, const int* frame_off, const int* pool_off, float* x0, float* stats, float* gstat,
                         float* part, int pstride, int B, int max_frames, int n_mels, int Mp, hipStream_t st, float* amax_out) {
    const bool card = n_mels == 128;
    if (max_frames <= kMelClipFrames) {
        if (card)
            hipLaunchKernelGGL(mel_norm_clip_fwd_kernel, dim3(B), dim3(512), 0, st, xm, frame_off, pool_off, x0, stats, gstat, amax_out);
        else
            hipLaunchKernelGGL(mel_any_clip_fwd_kernel, dim3(B), dim3(512), 0, st, xm, frame_off, pool_off, x0, stats, gstat, n_mels, Mp);
        return;
    }
    if (card)
        mel_chunked_fwd<MelBank128>(xm, frame_off, pool_off, x0, stats, gstat, part, pstride, B, max_frames, n_mels, Mp, st);
    else
        mel_chunked_fwd<MelBankAny>(xm, frame_off, pool_off, x0, stats, gstat, part, pstride, B, max_frames, n_mels, Mp, st);
}
void launch_mel_norm_bwd(const float* dx0, float* xm, const int* frame_off, const int* pool_off, const float* stats,
                         const float* gstat, float* part, int pstride, int B, int max_frames, int n_mels, int Mp, hipStream_t st) {
    const bool card = n_mels == 128;
    if (max_frames <= kMelClipFrames) {
        if (card)
            hipLaunchKernelGGL(mel_norm_clip_bwd_kernel, dim3(B), dim3(512), 0, st, dx0, xm, frame_off, pool_off, stats, gstat);
        else
            hipLaunchKernelGGL(mel_any_clip_bwd_kernel, dim3(B), dim3(512), 0, st, dx0, xm, frame_off, pool_off, stats, gstat, n_mels, Mp);
        return;
    }
    if (card)
        mel_chunked_bwd<MelBank128>(dx0, xm, frame_off, pool_off, stats, gstat, part, pstride, B, max_frames, n_mels, Mp, st);
    else
        mel_chunked_bwd<MelBankAny>(dx0, xm, frame_off, pool_off, stats, gstat, part, pstride, B, max_frames, n_mels, Mp, st);
}
void launch_head(const float* a3, const int* frame_off, const int* pool_off, const float* target, float* pred, float* loss,
                 float* best_loss, int* improved, float* dA3, int* step, int loss_kind, int nbits, int B,
                 hipStream_t st, const float* loss_add, int final_act, int C, TapRows rows) {
    if (C < 2 * nbits) C = 2 * nbits;
#define AW_HEAD_P(FA, P)                                                                                                    \
    hipLaunchKernelGGL((head_kernel<FA, P>), dim3(B), dim3(256), 0, st, a3, frame_off, pool_off, target, pred, loss, best_loss, \
                       improved, dA3, step, loss_kind, nbits, loss_add, C, rows)
#define AW_HEAD(FA) do { if (rows.pooled()) AW_HEAD_P(FA, true); else AW_HEAD_P(FA, false); } while (0)
    switch (final_act) {
        case kActRelu: AW_HEAD(kActRelu); break;
        case kActLRelu: AW_HEAD(kActLRelu); break;
        case kActGelu: AW_HEAD(kActGelu); break;
        case kActSwish: AW_HEAD(kActSwish); break;
        case kActSigmoid: AW_HEAD(kActSigmoid); break;
        default: AW_HEAD(kActTanh); break;
    }
#undef AW_HEAD
#undef AW_HEAD_P
}

}  // namespace aware
