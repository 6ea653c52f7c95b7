// Attack mixtures (EXTENSION, parity unpinned: the reference has no attacks in its loop): one of several loop chains drawn per
// clip and optimiser step.  DESIGN.md section 22; the host twin is aware_amd/embedding/loop_attacks.py::mixture_choice.
//
//   r = philox4x32_10((0, s, 12, 1), (seed_b, 0x5EED))          word 12: the entries' draws are words 1..4, the noise word 0,
//                                                               the impulse responses word 8
//   T_c = min(floor((w_0 + .. + w_c) 2^32), 2^32), the float32 weights summed in double
//   choice_b = the first c with r[0] < T_c, or -1
//
// s is the optimiser step read from device memory, so a recorded graph replays with fresh draws.  The kernel runs at the top of
// every loop body; every kernel of the loop family then reads choice[] through its gate (common.hpp, LoopGate), in the forward
// and in the backward half, so the backward half sees the forward half's choice whatever the step counter has become.
#include <cmath>

#include "common.hpp"
#include "kernels.h"
#include "loop_rng.hpp"

namespace aware {

namespace {

__global__ __launch_bounds__(64) void loop_mix_draw_kernel(LoopMixDrawLaunch a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const unsigned step = (unsigned)(a.step ? *a.step : a.step_imm);
    unsigned r[4];
    philox4x32_10(0u, step, 12u, 1u, a.seeds[b], 0x5EEDu, r);
    int c = -1;
#pragma unroll
    for (int j = kMaxLoopChains - 1; j >= 0; --j)
        if (j < a.n && (unsigned long long)r[0] < a.thr[j]) c = j;
    a.choice[b] = c;
}

}  // namespace

void launch_loop_mix_draw(const LoopMixDrawLaunch& L, hipStream_t st) {
    hipLaunchKernelGGL(loop_mix_draw_kernel, dim3((unsigned)((L.B + 63) / 64)), dim3(64), 0, st, L);
}

}  // namespace aware
