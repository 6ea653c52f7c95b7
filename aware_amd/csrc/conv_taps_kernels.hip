// Unfold and fold of the detector's temporal convolutions (conv_taps.hpp).  A block's Conv1d over k taps
// is the plain GEMM of the unfolded rows U [NP][k Cs] with the weights laid out [C_out][k Cs]; its data gradient is the GEMM to
// dU followed by the fold.  Both kernels only move data: float4 along the channel axis, coalesced along the k Cs axis of U, no
// LDS.  Zero padding is decided per clip from its own row count, so a clip never reads its neighbour's rows -- also where its
// rows end exactly on the 32-row boundary the next clip starts at.
#include "conv_taps.hpp"

namespace aware {

constexpr int kTapRowsPerBlock = 8;

// grid (row tiles of the longest clip, B), 256 threads: a tile of kTapRowsPerBlock rows of U, walked float4 by float4
template <bool POOL>
__global__ __launch_bounds__(256) void conv_unfold_kernel(const float* __restrict__ X, float* __restrict__ U,
                                                          const int* __restrict__ frame_off, const int* __restrict__ pool_off,
                                                          int Cs, int layer, int k, int s, int p, int psize, int pstride) {
    const int b = blockIdx.y;
    const int r0 = pool_off[b], rows = pool_off[b + 1] - r0;            // the clip's rows up to its 32-row boundary
    const int t0 = blockIdx.x * kTapRowsPerBlock;
    if (t0 >= rows) return;
    const int T = frame_off[b + 1] - frame_off[b];
    const int L0 = POOL ? pool_rows(T, psize, pstride) : T / 2;
    const int Lin = conv_rows(L0, layer, k, s, p), Lout = conv_rows(L0, layer + 1, k, s, p);
    const int C4 = Cs >> 2, W4 = k * C4;
    const int nt = rows - t0 < kTapRowsPerBlock ? rows - t0 : kTapRowsPerBlock;
    const float4* x4 = reinterpret_cast<const float4*>(X) + (size_t)r0 * C4;
    float4* u4 = reinterpret_cast<float4*>(U) + (size_t)(r0 + t0) * W4;
    for (int i = threadIdx.x; i < nt * W4; i += 256) {
        const int t = t0 + i / W4, col = i % W4;
        const int j = col / C4, c = col % C4;
        const int src = t * s - p + j;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < Lout && src >= 0 && src < Lin) v = x4[(size_t)src * C4 + c];
        u4[i] = v;
    }
}

// grid (row tiles of the longest clip, B), 256 threads: a tile of kTapRowsPerBlock rows of dX; every value the sum of at most
// k values of dU, taken j ascending
template <bool POOL>
__global__ __launch_bounds__(256) void conv_fold_kernel(const float* __restrict__ dU, float* __restrict__ dX,
                                                        const int* __restrict__ frame_off, const int* __restrict__ pool_off,
                                                        int Cs, int layer, int k, int s, int p, int psize, int pstride) {
    const int b = blockIdx.y;
    const int r0 = pool_off[b], rows = pool_off[b + 1] - r0;
    const int q0 = blockIdx.x * kTapRowsPerBlock;
    if (q0 >= rows) return;
    const int T = frame_off[b + 1] - frame_off[b];
    const int L0 = POOL ? pool_rows(T, psize, pstride) : T / 2;
    const int Lin = conv_rows(L0, layer, k, s, p), Lout = conv_rows(L0, layer + 1, k, s, p);
    const int C4 = Cs >> 2, W4 = k * C4;
    const int nq = rows - q0 < kTapRowsPerBlock ? rows - q0 : kTapRowsPerBlock;
    const float4* u4 = reinterpret_cast<const float4*>(dU) + (size_t)r0 * W4;
    float4* x4 = reinterpret_cast<float4*>(dX) + (size_t)(r0 + q0) * C4;
    for (int i = threadIdx.x; i < nq * C4; i += 256) {
        const int q = q0 + i / C4, c = i % C4;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < Lin) {
            for (int j = 0; j < k; ++j) {
                const int e = q + p - j;
                if (e < 0 || e % s) continue;
                const int t = e / s;
                if (t >= Lout) continue;
                const float4 v = u4[(size_t)t * W4 + j * C4 + c];
                a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
            }
        }
        x4[i] = a;
    }
}

static dim3 tap_grid(int B, int max_pooled) {
    const int rows = (max_pooled + 31) & ~31;
    return dim3((rows + kTapRowsPerBlock - 1) / kTapRowsPerBlock, B);
}

void launch_conv_unfold(const float* X, float* U, const int* frame_off, const int* pool_off, int Cs, int B, int max_pooled,
                        int layer, int k, int s, int p, hipStream_t st, int psize, int pstride) {
    if (B < 1 || max_pooled < 1) return;
    if (psize != 2 || pstride != 2)
        hipLaunchKernelGGL(conv_unfold_kernel<true>, tap_grid(B, max_pooled), dim3(256), 0, st, X, U, frame_off, pool_off, Cs, layer,
                           k, s, p, psize, pstride);
    else
        hipLaunchKernelGGL(conv_unfold_kernel<false>, tap_grid(B, max_pooled), dim3(256), 0, st, X, U, frame_off, pool_off, Cs, layer,
                           k, s, p, 2, 2);
}

void launch_conv_fold(const float* dU, float* dX, const int* frame_off, const int* pool_off, int Cs, int B, int max_pooled,
                      int layer, int k, int s, int p, hipStream_t st, int psize, int pstride) {
    if (B < 1 || max_pooled < 1) return;
    if (psize != 2 || pstride != 2)
        hipLaunchKernelGGL(conv_fold_kernel<true>, tap_grid(B, max_pooled), dim3(256), 0, st, dU, dX, frame_off, pool_off, Cs, layer,
                           k, s, p, psize, pstride);
    else
        hipLaunchKernelGGL(conv_fold_kernel<false>, tap_grid(B, max_pooled), dim3(256), 0, st, dU, dX, frame_off, pool_off, Cs, layer,
                           k, s, p, 2, 2);
}

}  // namespace aware
