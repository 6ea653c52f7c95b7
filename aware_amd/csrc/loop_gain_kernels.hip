// Gain envelope (EXTENSION, parity unpinned: the reference has no attack of the kind and no chain inside its loop): a gain that
// moves over time, piecewise linear between random breakpoints P samples apart -- a fade, ducking, tremolo, an AGC riding the
// level.  DESIGN.md section 24; the torch restatement is aware_amd/embedding/loop_attacks.py::gain_envelope / apply_chain.
//
// Inside the embed loop the kind (8) is element-wise and lives in the stage kernels of loop_attack_kernels.hip.  This file is
// the operator alone on a ragged batch (aware_gain_envelope): always on, the draw of chain entry `entry` at step `step`.  One
// workgroup per kEnvSpan samples of a clip, with the breakpoint table and the division-free evaluation of loop_gain.hpp; one
// float per thread and step, so any offset is served and a wave reads and writes 256 consecutive bytes.  out may be in: every
// sample is read once by the thread that writes it.  Forward and adjoint are the same operator.
#include "common.hpp"
#include "kernels.h"
#include "loop_gain.hpp"

namespace aware {

namespace {

constexpr int kGeThreads = 256;

__global__ __launch_bounds__(kGeThreads) void gain_envelope_kernel(GainLaunch a) {
    __shared__ float gtab[kEnvTab];
    const int b = blockIdx.y;
    const int n = a.len[b];
    const int i0 = blockIdx.x * kEnvSpan;
    if (i0 >= n) return;
    const int i1 = min(i0 + kEnvSpan, n);
    const unsigned seed = a.seeds[b];
    unsigned r[4];
    philox4x32_10(0u, (unsigned)a.step, 1u + (unsigned)a.entry, 1u, seed, 0x5EEDu, r);
    int P, ph;
    envelope_draw(r, a.p_lo, a.p_hi, P, ph);
    const EnvBlock eb = envelope_block(gtab, i0, P, ph, a.floor, (unsigned)a.step, (unsigned)a.entry, seed);
    __syncthreads();
    const float* x = a.in + a.off[b];
    float* y = a.out + a.off[b];
    float* gout = a.gains ? a.gains + a.off[b] : nullptr;
    for (int i = i0 + threadIdx.x; i < i1; i += kGeThreads) {
        int kl, rem;
        envelope_locate(eb, i - i0, kl, rem);
        const float g = envelope_gain(eb, gtab, kl, rem);
        y[i] = x[i] * g;
        if (gout) gout[i] = g;
    }
}

}  // namespace

void launch_gain_envelope(const GainLaunch& L, hipStream_t st) {
    const unsigned gx = (unsigned)((L.max_len + kEnvSpan - 1) / kEnvSpan);
    hipLaunchKernelGGL(gain_envelope_kernel, dim3(gx, (unsigned)L.B, 1), dim3(kGeThreads), 0, st, L);
}

}  // namespace aware
