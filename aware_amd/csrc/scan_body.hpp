// The bodies of the two scan kernels (scan_kernels.hip), apart from the launch indices, so that tests/host_sim/scan_check.cpp
// can compile the same text for the host: it defines SCAN_HOST_SIM and supplies threadIdx, blockIdx, wave_sum, __ballot,
// __popcll, __popc, __syncthreads and the rounding intrinsics before it includes this header.  DESIGN.md section 28; the
// restatement is aware_amd/detection/sync.py (scan_select, scan_segments).
#pragma once

#ifndef SCAN_HOST_SIM
#define SCAN_FN __device__ __forceinline__
#define SCAN_SHARED __shared__
#endif

namespace aware {

#ifdef SCAN_HOST_SIM
constexpr int kScanMaxBits = 512;                      // as kernels.h has it
#endif
constexpr int kScanThreads = 256;                      // scan_segments_kernel: four waves per file
constexpr int kScanWaves = kScanThreads / 64;
constexpr int kScanRows = kScanMaxBits / 64;           // values of a row per lane

// ---- scan_select: one wave per window ------------------------------------------------------------------------------------------
//   c_j = mean_l |v[w][j][l] - centre| in sync_select_kernel's order (lane t adds l = t, t + 64, ... in ascending order, one
//   butterfly, one division), j* = the smallest j with the largest c_j (c > best from -1: a NaN row never wins),
//   win_conf[w] = c_j*, win_view[w] = j*, win_values[w] = v[w][j*], bit l of win_bits[w] = v[w][j*][l] > centre.
SCAN_FN void scan_select_body(const float* __restrict__ values, int n, int L, float centre, float* __restrict__ win_conf,
                              int* __restrict__ win_view, float* __restrict__ win_values, unsigned* __restrict__ win_bits) {
    const int w = blockIdx.x, t = threadIdx.x;
    const float* v = values + (size_t)w * n * L;
    float best = -1.f;
    int arg = 0;
    for (int j = 0; j < n; ++j) {
        const float* row = v + (size_t)j * L;
        float s = 0.f;
        for (int l = t; l < L; l += 64) s += fabsf(row[l] - centre);
        const float c = wave_sum(s) / (float)L;
        if (c > best) { best = c; arg = j; }        // all lanes hold the same c
    }
    const float* row = v + (size_t)arg * L;
    const int words = (L + 31) / 32;
    for (int l0 = 0; l0 < L; l0 += 64) {            // uniform trip count: every lane votes
        const int l = l0 + t;
        const float x = l < L ? row[l] : centre;
        if (l < L) win_values[(size_t)w * L + l] = x;
        const unsigned long long m = __ballot(x > centre);
        const int word = l0 / 32 + t;               // lanes 0 and 1 store the two halves of the vote
        if (t < 2 && word < words) win_bits[(size_t)w * words + word] = (unsigned)(m >> (32 * t));
    }
    if (t == 0) { win_view[w] = arg; win_conf[w] = best; }
}

// Window i of a file (w0 its first window) is marked.
SCAN_FN bool scan_marked(const float* __restrict__ win_conf, int w0, int i, float min_conf) { return win_conf[w0 + i] >= min_conf; }

// Window i > 0 opens a run although i - 1 is marked as well: their bits differ in more than max_flip places.
SCAN_FN bool scan_flipped(const unsigned* __restrict__ win_bits, int words, int w0, int i, int max_flip) {
    const unsigned* a = win_bits + (size_t)(w0 + i) * words;
    const unsigned* b = a - words;
    int flips = 0;
    for (int k = 0; k < words; ++k) flips += __popc(a[k] ^ b[k]);
    return flips > max_flip;
}

// ---- scan_segments: one workgroup of 256 threads per file ------------------------------------------------------------------------
// Pass one: thread i of every chunk of 256 windows decides whether its window opens a run; the inclusive count of the
// openings (a ballot and a popcount per wave, the four wave totals and the carry of the chunks before in LDS) is the
// window's run number.  The window that opens run r < max_segments stores seg_first[r], the one that closes it seg_last[r].
// Pass two: wave v takes the runs v, v + 4, ... and walks each run's windows in ascending order, lanes over l, the weighted
// sums in registers: one fixed order, no atomics.  Slots beyond the run count are not written.
SCAN_FN void scan_segments_body(const float* __restrict__ win_conf, const int* __restrict__ win_view,
                                const float* __restrict__ win_values, const unsigned* __restrict__ win_bits,
                                const int* __restrict__ win_off, int L, float centre, float min_conf, int max_flip,
                                int max_segments, int* __restrict__ n_seg, int* __restrict__ seg_first,
                                int* __restrict__ seg_last, int* __restrict__ seg_peak, int* __restrict__ seg_view,
                                float* __restrict__ seg_conf, float* __restrict__ seg_values) {
    SCAN_SHARED int wave_total[kScanWaves];
    SCAN_SHARED int carry;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int w0 = win_off[b], nw = win_off[b + 1] - w0, words = (L + 31) / 32;
    int* first = seg_first + (size_t)b * max_segments;
    int* last = seg_last + (size_t)b * max_segments;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int i0 = 0; i0 < nw; i0 += kScanThreads) {        // uniform trip count: every thread reaches the barriers
        const int i = i0 + t;
        bool marked = false, opens = false, closes = false;
        if (i < nw) {
            marked = scan_marked(win_conf, w0, i, min_conf);
            if (marked) {
                opens = i == 0 || !scan_marked(win_conf, w0, i - 1, min_conf) || scan_flipped(win_bits, words, w0, i, max_flip);
                closes = i == nw - 1 || !scan_marked(win_conf, w0, i + 1, min_conf) ||
                         scan_flipped(win_bits, words, w0, i + 1, max_flip);
            }
        }
        const unsigned long long m = __ballot(opens);
        if (lane == 0) wave_total[wave] = __popcll(m);
        __syncthreads();
        int run = carry + __popcll(m & (~0ull >> (63 - lane)));      // inclusive within the wave
        for (int k = 0; k < wave; ++k) run += wave_total[k];
        if (marked && run <= max_segments) {               // run numbers count from 1 here
            if (opens) first[run - 1] = i;
            if (closes) last[run - 1] = i;
        }
        __syncthreads();                                   // everyone has read carry and the totals
        if (t == 0) {
            int sum = carry;
            for (int k = 0; k < kScanWaves; ++k) sum += wave_total[k];
            carry = sum;
        }
        __syncthreads();
    }
    const int total = carry;
    if (t == 0) n_seg[b] = total;
    const int runs = total < max_segments ? total : max_segments;
    for (int r = wave; r < runs; r += kScanWaves) {
        const int a = first[r], z = last[r];               // stored by this workgroup before the last barrier
        float num[kScanRows];
#pragma unroll
        for (int k = 0; k < kScanRows; ++k) num[k] = 0.f;
        float den = 0.f, best = win_conf[w0 + a];
        int peak = a;
        for (int i = a; i <= z; ++i) {
            const float c = win_conf[w0 + i];
            const float* row = win_values + (size_t)(w0 + i) * L;
            if (c > best) { best = c; peak = i; }          // the smallest window with the largest confidence
            den = __fadd_rn(den, c);
#pragma unroll
            for (int k = 0; k < kScanRows; ++k) {
                const int l = lane + 64 * k;
                if (l < L) num[k] = __fadd_rn(num[k], __fmul_rn(c, __fsub_rn(row[l], centre)));   // unfused, as stated
            }
        }
        float* out = seg_values + ((size_t)b * max_segments + r) * L;
#pragma unroll
        for (int k = 0; k < kScanRows; ++k) {
            const int l = lane + 64 * k;
            if (l < L) out[l] = __fadd_rn(centre, __fdiv_rn(num[k], den));
        }
        if (lane == 0) {
            const size_t s = (size_t)b * max_segments + r;
            seg_peak[s] = peak; seg_view[s] = win_view[w0 + peak]; seg_conf[s] = best;
        }
    }
}

}  // namespace aware
