// What the chunked family of the detector's mel stage shares between its two files: detector_kernels.hip (the (2, 2) pool of
// the model card) and mel_pool_kernels.hip (any other initial pool).  The maths is mel_norm.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include "common.hpp"
#include "mel_norm.hpp"

namespace aware {

// every wave's sum of v into red[wave]
__device__ __forceinline__ void wave_partials(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
}
// 256 threads (the four partials in sequence: the pairwise order of mel_sum8 would change the bits of every caller)
__device__ __forceinline__ float block_sum(float v, float* red) {
    wave_partials(v, red);
    return red[0] + red[1] + red[2] + red[3];
}

// A bank of n_mels <= 512 bands in rows of Mp >= n_mels floats, taken in groups of 128 channels (the family's comment in
// detector_kernels.hip).  MelBank128 makes the card's 128 bands, pitch and single group compile-time constants; MelBankAny
// takes them at run time.
struct MelBank128 {
    static constexpr int kGroups = 1;
    static constexpr int n_mels = 128, Mp = 128, ng = 1;
    __device__ MelBank128(int, int) {}
};
struct MelBankAny {
    static constexpr int kGroups = 4;               // 128-channel groups: Mp <= 512
    int n_mels, Mp, ng;
    __device__ MelBankAny(int n_mels_, int Mp_) : n_mels(n_mels_), Mp(Mp_), ng((Mp_ + 127) / 128) {}
};

// per-chunk (mean, M2) of every channel into part [B][pstride][2 Mp]: mel_partial_stats_kernel, which does not depend on the pool
void launch_mel_partial_stats(const float* xm, const int* frame_off, float* part, int pstride, int B, int max_frames, int n_mels,
                              int Mp, hipStream_t st);

}  // namespace aware
