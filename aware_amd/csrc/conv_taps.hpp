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

// The rows a norm / activation or read-out kernel works on: those of the clip behind `layer` blocks.  The default (layer 0) is
// the clip's pooled frames, what every detector of 1x1 convolutions has in every block.
struct TapRows {
    int layer = 0, k = 1, s = 1, p = 0;
    __host__ __device__ int of(int L0) const { return conv_rows(L0, layer, k, s, p); }
};

// ---- conv_taps_kernels.hip.  Activations are frame-major rows [NP][Cs] (Cs % 4 == 0); clip b starts at row pool_off[b]
// (32-aligned) in every block, and only the count of valid rows shrinks from block to block.
// unfold: U[r0 + t][j Cs + c] = X[r0 + t s - p + j][c] where 0 <= t s - p + j < L_in, else 0, for t < L_out (layer + 1 blocks);
// rows L_out .. the clip's 32-row boundary are written as zeros
void launch_conv_unfold(const float* X, float* U, const int* frame_off, const int* pool_off, int Cs, int B, int max_pooled,
                        int layer, int k, int s, int p, hipStream_t st);
// fold, the exact adjoint in gather form: dX[r0 + q][c] = sum over j ascending of dU[r0 + t][j Cs + c] with t s - p + j = q,
// 0 <= t < L_out, for q < L_in; rows L_in .. the clip's 32-row boundary are written as zeros
void launch_conv_fold(const float* dU, float* dX, const int* frame_off, const int* pool_off, int Cs, int B, int max_pooled,
                      int layer, int k, int s, int p, hipStream_t st);

}  // namespace aware
