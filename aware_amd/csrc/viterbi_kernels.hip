// Coded payloads (EXTENSION, no counterpart in the reference): the soft-decision Viterbi decoder of the constraint-length-7
// convolutional codes of utils/watermark/fec.py.  The code has 64 trellis states, one per lane: one wave decodes one row of
// detector outputs, four rows per workgroup, one launch over all rows.  The survivor bits of a step are one __ballot, kept in
// registers (lane t % 64 holds step t); no LDS, no atomics, no scratch.  DESIGN.md section 29; the restatement is
// aware_amd/utils/watermark/fec.py (viterbi_decode); the body is in viterbi_body.hpp.
#include "common.hpp"
#include "kernels.h"
#include "viterbi_body.hpp"

namespace aware {

namespace {

__global__ __launch_bounds__(64 * kViterbiRows) void viterbi_kernel(const float* __restrict__ values, int R, int L, float centre,
                                                                   int n, int c, unsigned* __restrict__ bits,
                                                                   float* __restrict__ metric, int* __restrict__ valid,
                                                                   int* __restrict__ corrected) {
    // the wave's number is the same in all its lanes: say so, and the row's address and the traceback stay on the scalar unit
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    viterbi_body(values, R, L, centre, n, c, (int)blockIdx.x, wave, bits, metric, valid, corrected);
}

}  // namespace

void launch_viterbi(const float* values, int R, int L, float centre, int n, int c, unsigned* bits, float* metric, int* valid,
                    int* corrected, hipStream_t st) {
    const unsigned groups = (unsigned)((R + kViterbiRows - 1) / kViterbiRows);
    hipLaunchKernelGGL(viterbi_kernel, dim3(groups), dim3(64 * kViterbiRows), 0, st, values, R, L, centre, n, c, bits, metric,
                       valid, corrected);
}

}  // namespace aware
