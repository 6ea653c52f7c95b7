// Temporal convolutions of the detector's blocks: Conv1d(C_in, C_out, k, stride s, padding p) along the
// pooled-frame axis of every block.  The one statement of the row rule, shared by the kernels and the host checks (Python mirror:
// runtime.py conv_rows).
#pragma once
#include <hip/hip_runtime.h>

namespace aware {

// what aware_detector_create_conv serves: 2 p <= k - 1, so that no block is longer than its input for any L >= 1 and every block
// fits the rows the batch allocates for the clip
constexpr int kMaxTapKernel = 7, kMaxTapStride = 4;

// rows of a clip of L0 pooled frames behind `layer` blocks: L -> floor((L + 2 p - k) / s) + 1 per block, 0 once a block has
// no output row (torch raises there; the entry points refuse such a clip before any launch).  layer = 0: L0 itself
__host__ __device__ inline int conv_rows(int L0, int layer, int k, int s, int p) {
    int L = L0;
    for (int i = 0; i < layer; ++i) {
        const int a = L + 2 * p - k;
        L = a < 0 ? 0 : a / s + 1;
    }
    return L;
}

// The initial pool between the mel stage and block 0: AvgPool1d(size, stride) along the frames.  What
// aware_detector_create_pool serves is size and stride 2..8 each: then pool_rows(T) <= floor(T / 2) for every T, so every clip
// fits the 32-aligned rows the batch tables allocate for it (batch_layout.hpp) whatever the pool is
constexpr int kMinPool = 2, kMaxPool = 8;

// rows of a clip of T frames behind the pool: floor((T - size) / stride) + 1, 0 for T < size (torch's AvgPool1d raises there;
// the entry points refuse such a clip before any launch).  pool_rows(T, 2, 2) == T / 2 for every T >= 0.  Python mirror:
// runtime.py pool_rows
__host__ __device__ inline int pool_rows(int T, int size, int stride) { return T < size ? 0 : (T - size) / stride + 1; }

// The rows a norm / activation or read-out kernel works on: those of the clip behind `layer` blocks.  The default (layer 0) is
// the clip's pooled frames, what every detector of 1x1 convolutions has in every block.  psize / pstride: the initial pool, for
// the kernels' pooled instantiations (kRowsPool), which take the clip's pooled frames from pool_rows; every other
// instantiation never looks at them.
struct TapRows {
    int layer = 0, k = 1, s = 1, p = 0;
    int psize = 2, pstride = 2;
    __host__ __device__ int of(int L0) const { return conv_rows(L0, layer, k, s, p); }
    __host__ __device__ bool pooled() const { return psize != 2 || pstride != 2; }
};
// how a kernel finds the rows of a clip of T frames: T / 2 (1x1 blocks after the (2, 2) pool; `rows` is never read),
// rows.of(T / 2) (temporal convolutions), rows.of(pool_rows(T, psize, pstride)) (any other initial pool, with or without them)
constexpr int kRowsHalf = 0, kRowsTaps = 1, kRowsPool = 2;
inline int rows_rule(const TapRows& r) { return r.pooled() ? kRowsPool : r.layer != 0 ? kRowsTaps : kRowsHalf; }
// the clip's pooled frames L_0 under a rule (the expressions of kRowsHalf / kRowsTaps are what they always were)
template <int RULE>
__device__ __forceinline__ int rows_l0(int T, const TapRows& r) {
    return RULE == kRowsPool ? pool_rows(T, r.psize, r.pstride) : T / 2;
}

// ---- conv_taps_kernels.hip.  Activations are frame-major rows [NP][Cs] (Cs % 4 == 0); clip b starts at row pool_off[b]
// (32-aligned) in every block, and only the count of valid rows shrinks from block to block.
// unfold: U[r0 + t][j Cs + c] = X[r0 + t s - p + j][c] where 0 <= t s - p + j < L_in, else 0, for t < L_out (layer + 1 blocks);
// rows L_out .. the clip's 32-row boundary are written as zeros
void launch_conv_unfold(const float* X, float* U, const int* frame_off, const int* pool_off, int Cs, int B, int max_pooled,
                        int layer, int k, int s, int p, hipStream_t st, int psize = 2, int pstride = 2);
// (psize / pstride: the detector's initial pool; other than 2 / 2 the clip's L_0 is pool_rows of its frames -- a separate
//  instantiation, so that the (2, 2) form keeps its code)
// fold, the exact adjoint in gather form: dX[r0 + q][c] = sum over j ascending of dU[r0 + t][j Cs + c] with t s - p + j = q,
// 0 <= t < L_out, for q < L_in; rows L_in .. the clip's 32-row boundary are written as zeros
void launch_conv_fold(const float* dU, float* dX, const int* frame_off, const int* pool_off, int Cs, int B, int max_pooled,
                      int layer, int k, int s, int p, hipStream_t st, int psize = 2, int pstride = 2);

}  // namespace aware
