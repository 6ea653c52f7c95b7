// Scanning long recordings (EXTENSION, parity unpinned: the reference reads one payload per clip): the detector reads a file
// in windows, every window at the n views of the offset search; scan_select_kernel keeps the most confident view of every
// window, scan_segments_kernel joins the marked windows of every file into runs and reads one payload per run.  Two launches
// over all files, no atomics, one fixed summation order.  DESIGN.md section 28; the restatement is
// aware_amd/detection/sync.py (scan_select, scan_segments); the bodies are in scan_body.hpp.
#include "common.hpp"
#include "kernels.h"
#include "scan_body.hpp"

namespace aware {

namespace {

__global__ __launch_bounds__(64) void scan_select_kernel(const float* __restrict__ values, int n, int L, float centre,
                                                         float* __restrict__ win_conf, int* __restrict__ win_view,
                                                         float* __restrict__ win_values, unsigned* __restrict__ win_bits) {
    scan_select_body(values, n, L, centre, win_conf, win_view, win_values, win_bits);
}

__global__ __launch_bounds__(kScanThreads) void scan_segments_kernel(
        const float* __restrict__ win_conf, const int* __restrict__ win_view, const float* __restrict__ win_values,
        const unsigned* __restrict__ win_bits, const int* __restrict__ win_off, int L, float centre, float min_conf, int max_flip,
        int max_segments, int* __restrict__ n_seg, int* __restrict__ seg_first, int* __restrict__ seg_last,
        int* __restrict__ seg_peak, int* __restrict__ seg_view, float* __restrict__ seg_conf, float* __restrict__ seg_values) {
    scan_segments_body(win_conf, win_view, win_values, win_bits, win_off, L, centre, min_conf, max_flip, max_segments, n_seg,
                       seg_first, seg_last, seg_peak, seg_view, seg_conf, seg_values);
}

}  // namespace

void launch_scan_select(const float* values, int W, int n, int L, float centre, float* win_conf, int* win_view,
                        float* win_values, unsigned* win_bits, hipStream_t st) {
    hipLaunchKernelGGL(scan_select_kernel, dim3((unsigned)W), dim3(64), 0, st, values, n, L, centre, win_conf, win_view,
                       win_values, win_bits);
}

void launch_scan_segments(const ScanSegments& S, hipStream_t st) {
    hipLaunchKernelGGL(scan_segments_kernel, dim3((unsigned)S.B), dim3(kScanThreads), 0, st, S.win_conf, S.win_view, S.win_values,
                       S.win_bits, S.win_off, S.L, S.centre, S.min_conf, S.max_flip, S.max_segments, S.n_seg, S.seg_first,
                       S.seg_last, S.seg_peak, S.seg_view, S.seg_conf, S.seg_values);
}

}  // namespace aware
