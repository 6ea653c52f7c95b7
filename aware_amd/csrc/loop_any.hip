// The band kernels of the embed / detect loop on a general plan (kernels.h, BandLaunch): between the general spectrum of
// stft_any.hip and the band rows the detector and the optimiser work on.  The card geometry keeps its own kernels, which
// do this work inside the transforms.
//
// Layout: a workgroup is 4 waves; a wave takes 64 adjacent band columns of one row, so the loads and stores of both sides
// are contiguous along the bin axis (512 bytes of spectrum, 256 bytes of band row per wave).  blockIdx.x walks the rows in
// fours, blockIdx.y the band row in 64-column chunks: no thread exists for a bin outside the band row, and the only idle
// lanes are the padding columns of the last chunk (fewer than 64).  Every kernel is one pass.
#include <hip/hip_runtime.h>
#include "common.hpp"
#include "dsp_args.hpp"
#include "kernels.h"

namespace aware {
namespace {

constexpr int kBandRows = 4;

// the row and band column of this thread; false: no such row
__device__ __forceinline__ bool band_thread(const BandLaunch& L, int& row, int& f) {
    row = blockIdx.x * kBandRows + threadIdx.y;
    f = blockIdx.y * 64 + threadIdx.x;
    return row < L.NF;
}

// EXACT: the magnitude (and BEGIN's unit phasor) by polar_exact (polar.hpp), exact for bins of any amplitude: the original
// audio's decomposition at begin and the magnitudes detection reads.  The loop's own launch keeps the plain form.
template <bool BEGIN, bool EXACT>
__global__ __launch_bounds__(256) void band_mag_kernel(BandLaunch L, const cf* __restrict__ spec, float* __restrict__ mag,
                                                       BandBegin G) {
    static_assert(EXACT || !BEGIN, "begin stores the exact decomposition");
    int row, f;
    if (!band_thread(L, row, f)) return;
    const size_t idx = (size_t)row * L.bstride + f;
    float mg = 0.f;
    cf u = mk(0.f, 0.f);
    if (f < L.nband) {
        const cf X = spec[(size_t)row * L.sstride + L.band_lo + f];
        if (EXACT) {
            const Polar p = polar_exact<HwMath>(X.x, X.y);
            mg = p.mag;
            if (BEGIN) u = (mg > 0.f) ? mk(p.ux, p.uy) : mk(1.f, 0.f);           // angle(0) = 0
        } else {
            mg = fast_sqrt(X.x * X.x + X.y * X.y);
        }
    }
    mag[idx] = mg;
    if (BEGIN) {
        reinterpret_cast<cf*>(G.unit)[idx] = u;
        float lo, hi;
        box_bounds(mg, G.ratio, lo, hi);
        G.coef[idx] = mg; G.lo[idx] = lo; G.hi[idx] = hi;
        G.mom[idx] = 0.f; G.vel[idx] = 0.f; G.best[idx] = mg; G.c0[idx] = mg;
    }
}

__global__ __launch_bounds__(256) void band_assemble_kernel(BandLaunch L, const float* __restrict__ coef,
                                                            const cf* __restrict__ unit, cf* __restrict__ spec) {
    int row, f;
    if (!band_thread(L, row, f) || f >= L.nband) return;
    const size_t idx = (size_t)row * L.bstride + f;
    const float c = coef[idx];
    const cf u = unit[idx];
    spec[(size_t)row * L.sstride + L.band_lo + f] = mk(c * u.x, c * u.y);
}

__global__ __launch_bounds__(256) void band_mag_bwd_kernel(BandLaunch L, const cf* __restrict__ spec,
                                                           const float* __restrict__ gmag, cf* __restrict__ gspec) {
    int row, f;
    if (!band_thread(L, row, f) || f >= L.nband) return;
    const size_t k = (size_t)row * L.sstride + L.band_lo + f;
    const cf X = spec[k];
    const float mg = fast_sqrt(X.x * X.x + X.y * X.y);
    const float s = (mg > 0.f) ? gmag[(size_t)row * L.bstride + f] * fast_rcp(mg) : 0.f;      // d|S| at S = 0: 0, as torch
    gspec[k] = mk(X.x * s, X.y * s);
}

// dL/dcoef of one bin: the gradient spectrum projected on the bin's unit phasor.  One fused form for both instantiations of
// the kernel below: left to the compiler, the stepping one contracted the sum into an FMA and the reporting one did not, so
// aware_embed_gradient reported a gradient whose last bit was not the one the step had consumed (the two terms cancel where
// the gradient is small, and NAdam's first steps turn 1e-11 there into 1e-3 of a coefficient).
__device__ __forceinline__ float coef_grad(cf G, cf u) { return __builtin_fmaf(G.x, u.x, G.y * u.y); }

template <bool STEP>
__global__ __launch_bounds__(256) void band_coef_grad_kernel(BandLaunch L, const cf* __restrict__ gspec,
                                                             const cf* __restrict__ unit, float* __restrict__ grad_out,
                                                             BandStep S) {
    int row, f;
    if (!band_thread(L, row, f) || f >= L.nband) return;
    const size_t idx = (size_t)row * L.bstride + f;
    const cf G = gspec[(size_t)row * L.sstride + L.band_lo + f];
    const cf u = unit[idx];
    const float g = coef_grad(G, u);
    if (grad_out) grad_out[idx] = g;
    if (STEP) {
        // the clip of this row (the same for the whole wave): frame_off[clip] <= row < frame_off[clip + 1]
        int lo_ = 0, hi_ = L.B;
        while (hi_ - lo_ > 1) {
            const int mid = (lo_ + hi_) >> 1;
            if (L.frame_off[mid] <= row) lo_ = mid; else hi_ = mid;
        }
        const float4 sc = reinterpret_cast<const float4*>(S.sched)[min(max(*S.step - 1, 0), S.sched_len - 1)];
        float p = S.coef[idx], mo = S.mom[idx], ve = S.vel[idx];
        nadam_clamp_update(p, mo, ve, g, S.lo[idx], S.hi[idx], sc.x, sc.y, 1.0f / sc.z,
                           make_float4(S.hyp[0], S.hyp[1], S.hyp[2], S.hyp[3]));
        S.coef[idx] = p; S.mom[idx] = mo; S.vel[idx] = ve;
        if (S.improved[lo_]) S.best[idx] = p;
    }
}

__global__ __launch_bounds__(256) void rescale_normalize_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                const int* __restrict__ off, const int* __restrict__ len,
                                                                const unsigned long long* __restrict__ pmax,
                                                                const int* __restrict__ pcount, int pstride,
                                                                const float* __restrict__ rescale) {
    __shared__ unsigned long long red[4];
    const int b = blockIdx.y;
    const ClipNorm cn = clip_norm_from_partials(pmax + (size_t)b * pstride, pcount[b], red);
    const int n = len[b];
    const float r = rescale ? rescale[b] : 1.f;
    const float* x = in + off[b];
    float* y = out + off[b];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) y[i] = r * (x[i] / cn.m);
}

inline dim3 band_grid(const BandLaunch& L) { return dim3((L.NF + kBandRows - 1) / kBandRows, L.bstride / 64); }
inline dim3 band_block() { return dim3(64, kBandRows); }

}  // namespace

void launch_band_mag(const BandLaunch& L, const void* spec, float* mag, const BandBegin* begin, bool exact, hipStream_t st) {
    if (begin) hipLaunchKernelGGL((band_mag_kernel<true, true>), band_grid(L), band_block(), 0, st, L, (const cf*)spec, mag, *begin);
    else if (exact) hipLaunchKernelGGL((band_mag_kernel<false, true>), band_grid(L), band_block(), 0, st, L, (const cf*)spec, mag, BandBegin());
    else hipLaunchKernelGGL((band_mag_kernel<false, false>), band_grid(L), band_block(), 0, st, L, (const cf*)spec, mag, BandBegin());
}

void launch_band_assemble(const BandLaunch& L, const float* coef, const void* unit, void* spec, hipStream_t st) {
    hipLaunchKernelGGL(band_assemble_kernel, band_grid(L), band_block(), 0, st, L, coef, (const cf*)unit, (cf*)spec);
}

void launch_band_mag_bwd(const BandLaunch& L, const void* spec, const float* gmag, void* gspec, hipStream_t st) {
    hipLaunchKernelGGL(band_mag_bwd_kernel, band_grid(L), band_block(), 0, st, L, (const cf*)spec, gmag, (cf*)gspec);
}

void launch_rescale_normalize(const float* in, float* out, const int* off, const int* len, const unsigned long long* pmax,
                              const int* pcount, int pstride, const float* rescale, int B, int max_len, hipStream_t st) {
    const int nx = max(1, (max_len + 1023) / 1024);
    hipLaunchKernelGGL(rescale_normalize_kernel, dim3(nx, B), dim3(256), 0, st, in, out, off, len, pmax, pcount, pstride, rescale);
}

void launch_band_coef_grad(const BandLaunch& L, const void* gspec, const void* unit, float* grad_out, const BandStep* step,
                           hipStream_t st) {
    if (step)
        hipLaunchKernelGGL(band_coef_grad_kernel<true>, band_grid(L), band_block(), 0, st, L, (const cf*)gspec, (const cf*)unit,
                           grad_out, *step);
    else
        hipLaunchKernelGGL(band_coef_grad_kernel<false>, band_grid(L), band_block(), 0, st, L, (const cf*)gspec,
                           (const cf*)unit, grad_out, BandStep());
}

}  // namespace aware
