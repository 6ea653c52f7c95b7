// Offset search in detection (EXTENSION, parity unpinned: the reference detects at the clip's own start only): of the n
// candidate views of a clip, keep the one the detector is most confident about.  DESIGN.md section 21; the restatement is
// aware_amd/detection/sync.py::sync_select.
//
//   c_j = mean_l |v[b][j][l] - centre|,  j* = the smallest j with the largest c_j,  out_values[b] = v[b][j*]
//
// One wave per clip.  Lane t adds the terms l = t, t + 64, ... in ascending order in f32, the 64 partial sums meet in one
// butterfly: one fixed order for every row, so equal rows give equal sums and an exact tie goes to the smaller j.
#include "common.hpp"
#include "kernels.h"

namespace aware {

namespace {

__global__ __launch_bounds__(64) void sync_select_kernel(const float* __restrict__ values, int n, int L, float centre,
                                                         float* __restrict__ out_values, int* __restrict__ out_index,
                                                         float* __restrict__ out_conf) {
    const int b = blockIdx.x, t = threadIdx.x;
    const float* v = values + (size_t)b * n * L;
    float best = -1.f;
    int arg = 0;
    for (int j = 0; j < n; ++j) {
        const float* row = v + (size_t)j * L;
        float s = 0.f;
        for (int l = t; l < L; l += 64) s += fabsf(row[l] - centre);
        const float c = wave_sum(s) / (float)L;
        if (c > best) { best = c; arg = j; }        // a NaN row never wins; all lanes hold the same c
    }
    const float* row = v + (size_t)arg * L;
    for (int l = t; l < L; l += 64) out_values[(size_t)b * L + l] = row[l];
    if (t == 0) { out_index[b] = arg; out_conf[b] = best; }
}

}  // namespace

void launch_sync_select(const float* values, int B, int n, int L, float centre, float* out_values, int* out_index,
                        float* out_conf, hipStream_t st) {
    hipLaunchKernelGGL(sync_select_kernel, dim3((unsigned)B), dim3(64), 0, st, values, n, L, centre, out_values, out_index,
                       out_conf);
}

}  // namespace aware
