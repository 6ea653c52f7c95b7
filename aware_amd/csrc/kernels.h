// Internal launch interface between the C ABI (capi.hip) and the kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "common.hpp"
#include "loop_limits.hpp"
#include "conv_taps.hpp"

namespace aware {

// ---- loop_mix_kernels.hip: attack mixtures (EXTENSION): one of several loop chains drawn per clip and step.  The gate every
// kernel of the loop family carries: with `choice` set, a workgroup whose clip did not draw chain `chain` returns at once
// (skipped, not copied); with `choice` null the kernel computes what it computes without a gate -------------------------
// (LoopGate, kMaxLoopChains and the other limits of the loop family are in loop_limits.hpp, which the host-only chain logic shares)
struct LoopMixDrawLaunch {
    const unsigned* seeds = nullptr;      // [B]
    const int* step = nullptr;            // device step counter, or null: step_imm
    int step_imm = 0, B = 0, n = 0;
    unsigned long long thr[kMaxLoopChains] = {0};     // T_c = min(floor((w_0 + .. + w_c) 2^32), 2^32)
    int* choice = nullptr;                // [B]
};
void launch_loop_mix_draw(const LoopMixDrawLaunch& L, hipStream_t st);

// ---- dsp_kernels.hip ------------------------------------------------------------------
constexpr int kStreamWaves = 4;        // waves (= runs) per workgroup of the streaming DSP kernels

struct AnalysisLaunch {
    PlanDev plan;
    const int* frame_off = nullptr;
    int B = 0, max_frames = 0;
    // streaming kernels: frames per run (0: chosen from B and max_frames) and the flat workgroup table of the batch
    // (entry = clip << 12 | workgroup within the clip; null: a (workgroups of the longest clip) x B grid)
    int run_frames = 0, n_wg = 0;
    const int* wg_tab = nullptr;
    const float* sig = nullptr;
    const int* sig_off = nullptr;
    const int* sig_len = nullptr;
    const unsigned long long* pmax = nullptr;
    const int* pcount = nullptr;
    int pstride = 0;
    int double_norm = 0;
    float unit_default = 0.f;
    int polar_exact = 0;              // forward, mag / unit: the kernel forms with polar_exact (polar.hpp), for the original audio
                                      // (begin, aware_stft_band).  0: the plain form of the loop's launches
    float* mag = nullptr;
    void* unit = nullptr;
    void* full = nullptr;
    // adjoint mode
    int adjoint = 0;
    const float* yraw = nullptr;
    const double* pdot = nullptr;
    const void* phasor = nullptr;
    float* coef = nullptr; float* mom = nullptr; float* vel = nullptr;
    const float* lo = nullptr; const float* hi = nullptr; float* best = nullptr;
    const int* improved = nullptr;
    const void* sched = nullptr;
    int sched_len = 0;
    const int* step = nullptr;
    float* grad_out = nullptr;
    int do_step = 0;
    float hyp[4] = {0.1f, 0.999f, 0.001f, 1e-8f};
    // stream = 1: barrier-free streaming wave kernels (dsp_stream.hip; narrow bands inside bins 1..256 and every wide band)
    int stream = 0;
    const float* gpad = nullptr;      // stream + adjoint: reflect-pad parts written by the streaming synthesis adjoint
    int write_pad = 1;                // stream, forward: write the zero tail of the mag / unit rows
    const float* c0 = nullptr;        // stream + adjoint: original coefficients (the box is recomputed from them)
    float box_ratio = 0.f;            // 10^(-tolerance_db / 20)
    float l1_weight = 0.f;            // != 0: L1 term on the coefficients (loss push_extremes + L1)
    float* mel_out = nullptr;         // stream, forward: the mel tile [NF][128] instead of mag (AnalysisArgs)
    const float* melf_w = nullptr;
    const unsigned char* melf_s = nullptr;
    LoopGate gate;                    // staged kernels on a full spectrum (the phase vocoder's stage inside a mixture)
};
struct SynthLaunch {
    PlanDev plan;
    const int* frame_off = nullptr;
    int B = 0, max_frames = 0;
    int n_wg = 0;
    const int* wg_tab = nullptr;        // as in AnalysisLaunch, for runs of run_blocks hop blocks
    const float* amp = nullptr;
    const void* ph = nullptr;
    const void* full = nullptr;
    float* out = nullptr;
    const float* add = nullptr;
    unsigned long long* pmax = nullptr;
    int pstride = 0;
    int adjoint = 0;
    const float* yraw = nullptr;
    const unsigned long long* pmax_in = nullptr;
    const int* pcount = nullptr;
    double* pdot = nullptr;
    int stream = 0;
    float* gpad = nullptr;            // stream + adjoint: [B][2][512] reflect-pad parts out
    int run_blocks = kSynthBlocks;    // hop blocks per run (aware_batch::synth_run); the partial counts follow it
    const float* c0 = nullptr;        // stream, forward: per-run sums of |amp - c0| into pl1 (L1 term)
    double* pl1 = nullptr;
    const int* sig_off = nullptr;     // staged adjoint on a full spectrum: general-length output (see SynthArgs)
    const int* sig_len = nullptr;
    const float* dmel = nullptr;      // stream + adjoint: amplitudes from dL/d(mel) [NF][128] through the two-tap table (SynthArgs)
    const void* melw = nullptr;
    const unsigned char* melm = nullptr;
    LoopGate gate;                    // staged kernels on a full spectrum (the phase vocoder's stage inside a mixture)
};
void launch_absmax_partials(const float* sig, const int* sig_off, const int* sig_len, unsigned long long* pmax,
                            int pstride, int B, int max_len, hipStream_t st);
void launch_analysis(const AnalysisLaunch& L, hipStream_t st);
void launch_synth(const SynthLaunch& L, hipStream_t st);
// dsp_stream.hip: true when the streaming wave kernels serve this plan (band inside bins 1..256)
bool stream_supported(const PlanDev& plan);
void launch_analysis_stream(const AnalysisLaunch& L, hipStream_t st);
void launch_synth_stream(const SynthLaunch& L, hipStream_t st);
// l1term[b] = weight * (sum of the clip's pl1 partials) / (nband * T_b): the L1 part of the loss push_extremes + L1
void launch_l1_reduce(const double* pl1, const int* pcount, int pstride, const int* frame_off, int nband, float weight,
                      float* l1term, int B, hipStream_t st);
void launch_embed_prepare(const float* c0, float* coef, float* lo, float* hi, float* mom, float* vel, float* best,
                          float* c0_keep, float ratio, size_t n, hipStream_t st);
void launch_oob_residual(const float* audio, const int* in_off, const unsigned long long* pmax, const int* pcount,
                         int pstride, const float* band, const int* frame_off, float* oob, int B, int max_frames,
                         hipStream_t st);
void launch_finish(const float* yraw, const int* frame_off, const unsigned long long* pmax, const int* pcount,
                   int pstride, const float* rescale, float* out, const int* out_off, int B, int max_frames,
                   hipStream_t st);

// ---- detector_kernels.hip ---------------------------------------------------------------
// C[M][N] = A[M][K] * Bt[N][K]^T (+ bias[N]); all row-major fp32, K % 4 == 0, 16-byte aligned rows
void launch_gemm_nt(const float* A, int lda, const float* Bt, int ldb, const float* bias, float* C, int ldc, int M,
                    int N, int K, hipStream_t st);
void launch_gemm_nt_variant(const float* A, int lda, const float* Bt, int ldb, const float* bias, float* C, int ldc,
                            int M, int N, int K, int variant, hipStream_t st);
int gemm_autotune(const float* A, int lda, const float* Bt, int ldb, float* C, int ldc, int M, int N, int K,
                  hipStream_t st);
// clip-aligned GEMM with fused InstanceNorm+LeakyReLU epilogues (uniform batches, <= 128 pooled rows per clip)
void launch_gemm_clip(const float* A, int lda, const float* Bt, int ldb, const float* bias, float* C, int ldc, int B,
                      int nwm, int Tp, int N, int K, int epi, float* rstd_io, const float* act, hipStream_t st);
// ---- gemm_x3.hip: the same clip-aligned GEMM on the bf16 matrix pipe, f32-equivalent (3-way operand split) ----
size_t x3_packed_bytes(int N, int K);
void x3_pack(const float* Wt, int N, int K, uint16_t* out);      // host: [N][K] f32 -> fragment-ordered bf16 planes
void launch_x3_pack_dev(const float* Wt_dev, int ldw, int Nvalid, int Kvalid, int N, int K, void* out, hipStream_t st);   // device -> device
bool gemm_clip_x3_supported(int nwm, int N, int K, int lda);
// mel projection + InstanceNorm + GlobalStandardize + AvgPool of a UNIFORM batch of clips of T <= 192 frames in one launch
// (one workgroup per clip): xm [NF][128] raw mel tile (kept for the backward), x0 pooled tile, stats / gstat as
// mel_norm.hpp lays them out
bool mel_front_x3_supported(int T, int K, int lda);
void launch_mel_front_x3(const float* mag, int lda, const void* melTpk, const int* frame_off, const int* pool_off, float* xm,
                         float* x0, float* stats, float* gstat, int B, int T, int K, hipStream_t st, float* amax_out = nullptr);
// (amax_out: [B][64], 8 partial maxima of |x0| per clip for gemm_h2.hip, or null)
// backward of the same block for the same batches: data gradient of the first conv block (dZ [NP][K], wTpk = x3_pack of its
// transposed weights [128][K]) + AvgPool / GlobalStandardize / InstanceNorm backward; xm: raw mel in, dL/d(mel) out
void launch_mel_back_x3(const float* dZ, int lda, const void* wTpk, const int* frame_off, const int* pool_off, float* xm,
                        const float* stats, const float* gstat, int B, int T, int K, hipStream_t st);
// lastpk/zpart (forward epilogue only): also emit the split-K partials [N/128][B*32*nwm][CL] of the next, last conv
// block (x3_pack of its weights zero-padded to a multiple of 16 rows), consumed by launch_readout_x3
void launch_gemm_clip_x3(const float* A, int lda, const void* Bpk, const float* bias, float* C, int ldc, int B, int nwm,
                         int Tp, int N, int K, int epi, float* rstd_io, const float* act, hipStream_t st,
                         const void* lastpk = nullptr, float* zpart = nullptr, int CL = 0, int Mrows = 0);
// ---- gemm_h2.hip: the same block on the f16 matrix pipe, two-term operand split, three products (f32-level) ----
size_t h2_packed_bytes(int N, int K);
void launch_h2_pack(const float* Wt_dev, int ldw, int N, int K, void* out, hipStream_t st);   // device -> device
void launch_clip_amax(const float* A, int lda, int K, int rows_per_clip, int B, float* amax, hipStream_t st);
bool gemm_clip_h2_supported(int nwm, int N, int K, int lda);
// the wide form: 4 waves x 64 columns per workgroup (tile = 2 below) instead of 8 waves x 16 (tile = 1); same bits
constexpr int kH2WideTile = 256;
bool gemm_clip_h2_wide_supported(int nwm, int N, int K, int lda);
// the form launch_gemm_clip_h2 takes for these arguments: 1 = 128-column, 2 = wide with the accumulator-layout epilogue,
// 3 = wide with the row-major epilogue (ldc % 4 == 0, C and act 16-byte aligned); epi 0..2, last: epi 1 with lastpk / zpart
int gemm_clip_h2_form(int tile, int nwm, int epi, bool last, const float* C, int ldc, const float* act);
// amax_in: [B][64] partial maxima of |A| per clip (K/16 valid); amax_out: [B][64] the same of C (N/16 written) or null
void launch_gemm_clip_h2(const float* A, int lda, const void* Bpk, const float* amax_in, float* amax_out, const float* bias,
                         float* C, int ldc, int B, int nwm, int Tp, int N, int K, int epi, float* rstd_io, const float* act,
                         hipStream_t st, const void* lastpk = nullptr, float* zpart = nullptr, int CL = 0, int tile = 1);
void launch_gemm_ragged_h2(const float* A, int lda, const void* Bpk, const float* amax_in, float* amax_out, const float* bias,
                           float* C, int ldc, int B, const int* frame_off, const int* pool_off, const int* order, int N, int K,
                           int epi, float* rstd_io, const float* act, hipStream_t st);
void launch_ragged_amax(const float* A, int lda, int K, const int* frame_off, const int* pool_off, int B, float* amax, hipStream_t st);
// (Mrows > 0, plain epilogue only: the matrices have Mrows < B*32*nwm rows -- the last row block is partial)
// the same block for ragged batches / clips of any length (one launch; clips longer than 96 pooled frames in two passes)
void launch_gemm_ragged_x3(const float* A, int lda, const void* Bpk, const float* bias, float* C, int ldc, int B,
                           const int* frame_off, const int* pool_off, const int* order, int N, int K, int epi, float* rstd_io,
                           const float* act, hipStream_t st);
// (order: [B] clip indices, longest first, or null = as given; speed only)
// fused read-out of the embed loop: last conv block + BRH + loss + their backward + data gradient of the last conv
// + backward of the previous block's norm/activation (uniform batches; see gemm_x3.hip)
bool readout_x3_supported(int nwm, int ci, int C);
void launch_readout_x3(const float* hin, int ci, const float* zpart, int nslab, const float* bias, const void* WTpk,
                       const float* rstd_prev, const float* target, float* pred, float* loss, float* best_loss, int* improved,
                       int* step, float* dZ, int B, int nwm, int Tp, int C, int nbits, int loss_kind, hipStream_t st,
                       const float* loss_add, void* img, float* amax_out = nullptr);
// (amax_out: [B][64], ci/16 partial maxima of |dZ| per clip for gemm_h2.hip, or null)
size_t readout_x3_image_bytes(int B, int nwm);      // scratch `img` of launch_readout_x3 (must not alias dZ)
// ragged batches: data gradient of the last conv from dZl (float32 rows, pitch 64, zero K padding: launch_tail with ldz = 64)
// with the backward of the previous block's InstanceNorm + LeakyReLU; ci % 128 == 0, last conv of at most 64 channels
void launch_readout_grad_ragged_x3(const float* hin, int ci, const float* dZl, const void* WTpk, const float* rstd_prev, float* dZ,
                                   const int* frame_off, const int* pool_off, const int* order, int B, hipStream_t st,
                                   float* amax_out = nullptr);
// mel block (mel_norm.hpp): InstanceNorm over time, per-clip GlobalStandardize, AvgPool(2,2), for a bank of n_mels <= 512 bands
// in rows of Mp >= n_mels floats (Mp % 4 == 0); stats [B][Mp][4], gstat [B][4], part [B][pstride][2 Mp] with pstride >=
// ceil(max_frames / 32).  Padding channels get zero statistics, zero x0 columns and zero dL/dxm.  Clips of up to kMelClipFrames
// frames take one workgroup per clip and leave part alone; longer clips a chunked form of two launches.  amax_out ([B][64], as
// launch_mel_front_x3) is written by the 128-band clip form only: det_plan hands it over where that form runs
constexpr int kMelClipFrames = 192;
void launch_mel_norm_fwd(const float* xm, const int* frame_off, const int* pool_off, float* x0, float* stats, float* gstat,
                         float* part, int pstride, int B, int max_frames, int n_mels, int Mp, hipStream_t st,
                         float* amax_out = nullptr);
void launch_mel_norm_bwd(const float* dx0, float* xm_inout, const int* frame_off, const int* pool_off, const float* stats,
                         const float* gstat, float* part, int pstride, int B, int max_frames, int n_mels, int Mp, hipStream_t st);
// ---- mel_pool_kernels.hip: the same stage for a detector with an initial pool other than (2, 2) -- AvgPool1d(size, stride),
// size and stride kMinPool..kMaxPool (conv_taps.hpp: pool_rows).  Same buffers; clips of every length take the chunked form
// (part is always written); x0 rows pool_rows(T) .. the clip's 32-row boundary are written as zeros
void launch_mel_pool_fwd(const float* xm, const int* frame_off, const int* pool_off, float* x0, float* stats, float* gstat,
                         float* part, int pstride, int B, int max_frames, int n_mels, int Mp, int size, int stride, hipStream_t st);
void launch_mel_pool_bwd(const float* dx0, float* xm_inout, const int* frame_off, const int* pool_off, const float* stats,
                         const float* gstat, float* part, int pstride, int B, int max_frames, int n_mels, int Mp, int size,
                         int stride, hipStream_t st);
// ---- architecture variants of the detector (aware_detector_arch; the values are the header's AWARE_ACT_* / AWARE_NORM_* /
// AWARE_FINAL_*): the norm and activation of every conv block and the read-out's final activation
constexpr int kActRelu = 0, kActLRelu = 1, kActGelu = 2, kActSwish = 3, kActTanh = 4, kActSigmoid = 5;
constexpr int kNormInstance = 0, kNormAffine = 1, kNormNone = 2;
// whether the backward of a block needs its pre-activation u (the norm's output) kept from the forward: every activation but
// LeakyReLU can not be inverted from its output, and the InstanceNorm backward needs u at every position (also where ReLU gave 0)
AW_HD constexpr bool norm_act_needs_stash(int norm, int act) {
    return !(act == kActLRelu || (act == kActRelu && norm != kNormInstance));
}
// conv block tail, in place on x [NP][C].  Forward: u = norm(x) (InstanceNorm over time, biased var, eps 1e-5; affine
// u = x * scale[c] + shift[c]; or identity), x = act(u).  Backward: x = dL/dA -> dL/dz, with u read from the stash or, where
// norm_act_needs_stash is false, recovered from the forward's output.  The defaults are the model card's block.
struct NormActLaunch {
    int norm = kNormInstance, act = kActLRelu;
    float* x = nullptr;
    const float* out = nullptr;           // backward without a stash: the forward's output A [NP][C]
    float* stash = nullptr;               // [NP][C] u: the forward writes it (null: not kept), the backward reads it
    float* rstd = nullptr;                // [B][C], InstanceNorm: the forward writes it, the backward reads it
    const float* scale = nullptr;         // [C] each, affine norm
    const float* shift = nullptr;
    const int* frame_off = nullptr;       // [B+1]
    const int* pool_off = nullptr;        // [B]: clip b's rows start at pool_off[b]
    int C = 0, B = 0, max_pooled = 0;
    // the block whose rows the kernel normalises, for a detector of temporal convolutions (conv_taps.hpp); the default is the
    // clip's pooled frames, and with it the kernels hold no trace of the row rule
    TapRows rows;
};
void launch_norm_act(const NormActLaunch& L, bool backward, hipStream_t st);
// BRH + loss + dL/dA3; also best-loss tracking.  final_act: kActRelu .. kActSigmoid applied to even - odd (the card: tanh)
void launch_head(const float* a3, const int* frame_off, const int* pool_off, const float* target, float* pred, float* loss,
                 float* best_loss, int* improved, float* dA3, int* step, int loss_kind, int nbits, int B,
                 hipStream_t st, const float* loss_add = nullptr, int final_act = kActTanh, int C = 0, TapRows rows = TapRows());
// (C: channel pitch of a3 / dA3; 0 = 2*nbits.  Channels 2*nbits .. C-1 are padding: never read out, dA3 zero)
void launch_gemm_nt_splitk(const float* A, int lda, const float* Bt, int ldb, float* Cpart, int ldc, int M, int N, int K,
                           int ksplit, hipStream_t st);
void launch_tail(const float* zpart, int nsplit, size_t slab, const float* bias, const int* frame_off, const int* pool_off,
                 const float* target, float* pred, float* loss, float* best_loss, int* improved, float* dZ, int* step,
                 int loss_kind, int nbits, int B, int max_pooled, hipStream_t st, const float* loss_add = nullptr, int ldz = 0,
                 int C = 0);
// (ldz: row pitch of dZ; 0 = C, 64 = zero-padded to the K of the bf16x3 data-gradient GEMM.  C: channel pitch of zpart;
//  0 = 2*nbits.  Channels 2*nbits .. C-1 are padding: never read out, dZ zero)

// wide read-out (64 < Cp <= 1024 channels, multiple of 128; 2*nbits of them read out): pred, and with a target the loss,
// best-loss bookkeeping and step counter as launch_head, and dout = dL/dA (staged route) or, card_bwd, dL/dZ of the card
// block with its InstanceNorm + LeakyReLU backward folded in (rstd of the block) plus gmax [B][64] partial maxima (or null)
void launch_readout_wide(const float* A, int Cp, const int* frame_off, const int* pool_off, const float* rstd, const float* target,
                         float* pred, float* loss, float* best_loss, int* improved, float* dout, float* gmax, int* step,
                         int loss_kind, int nbits, int B, hipStream_t st, const float* loss_add, int final_act, bool card_bwd,
                         TapRows rows = TapRows());

// ---- seam_kernels.hip: element-wise pieces of the differentiable plug-in seam -----------------------------
void launch_polar_decompose(const void* spec, float* mag, float* phase, size_t n, hipStream_t st);
void launch_polar_decompose_bwd(const void* spec, const float* gmag, const float* gphase, void* gspec, size_t n, hipStream_t st);
void launch_polar_assemble(const float* mag, const float* phase, void* spec, size_t n, hipStream_t st);
void launch_polar_assemble_bwd(const float* mag, const float* phase, const void* gspec, float* gmag, float* gphase, size_t n,
                               hipStream_t st);
void launch_transpose(const float* in, float* out, int R, int C, hipStream_t st);
void launch_colsum(const float* in, float* out, int R, int C, hipStream_t st);
void launch_normalize_bwd(const float* x, const float* g, float* dx, const int* off, const int* len, int B, hipStream_t st);
void launch_nadam_clamp(float* p, const float* g, float* m, float* v, const float* lo, const float* hi, size_t n, float c_grad,
                        float c_mom, float bias_corr2, float beta1, float beta2, float eps, hipStream_t st);

void launch_opt_clamp(int kind, float* p, const float* g, float* m, float* v, const float* lo, const float* hi, size_t n,
                      const float* c4, const float* h8, hipStream_t st);
void launch_opt_rows(int kind, float* coef, const float* grad, float* mom, float* vel, const float* c0, float ratio, float* best,
                     const int* improved, const int* frame_off, int B, int NF, const double* tab, int tab_len, const int* step,
                     const double* lr_clip, double wd, const float* h8, int nband, int stride, hipStream_t st);
void launch_plateau(const float* loss, double* state, double* lr_clip, int B, double factor, int patience, double threshold,
                    double min_lr, double eps, hipStream_t st);

// ---- attack_kernels.hip -----------------------------------------------------------------
void launch_pcm_quantize(const float* in, float* out, const int* off, const int* len, const unsigned long long* pmax,
                         const int* pcount, int pstride, float q, float lo, float hi, int B, int max_len,
                         hipStream_t st);
void launch_normalize(const float* in, float* out, const int* off, const int* len, const unsigned long long* pmax,
                      const int* pcount, int pstride, int B, int max_len, hipStream_t st);
void launch_upfirdn(const float* in, const int* in_off, const int* in_len, float* out, const int* out_off,
                    const int* out_len, const float* h, int nh, int up, int down, int half_len, int B, int max_out,
                    hipStream_t st);
void launch_iir_full(const float* in, const int* off, const int* len, void* out, int out_f64, const double* b,
                     const double* a, const double* zi, int ncoef, int mode, double* scratch, int sstride, int B,
                     hipStream_t st);
void launch_gaussian_noise_full(const float* in, float* out, const int* off, const int* len, const unsigned* seeds,
                                double* power, float snr_db, int B, int max_len, hipStream_t st);
void launch_snr(const float* a, const int* a_off, const float* b, const int* b_off, const int* len, double* out, int B,
                hipStream_t st);
void launch_phase_vocoder(const void* in, const int* fin, void* out, const int* fout, double rate, int B, hipStream_t st);
void launch_spectral_quantize(void* spec, int nframes, float step_db, float floor_db, hipStream_t st);
void launch_spectral_quantize_bwd(const void* spec, const void* gout, void* gin, int nframes, float step_db, float floor_db,
                                  hipStream_t st);
void launch_decimate_interp(const float* in, const int* off, const int* len, double* out, int k, int B, int max_len,
                            hipStream_t st);
void launch_segment_copy(const float* in, const int* in_off, float* out, const int* out_off, const int* out_len,
                         const int* cut_start, const int* cut_len, int zero_fill, int B, int max_len, hipStream_t st);

// ---- stft_any.hip: the general-geometry STFT path (any n_fft in 256..4096, hop, win_length) ------------------------
struct GenPlanDev {
    int n_fft = 0, hop = 0, stride = 0;   // stride: complex values per spectrum row (n_fft/2 + 1 rounded up to 8)
    const cf* th = nullptr;               // W_M^j = exp(-2 pi i j / M), j < M/2 (M = n_fft/2)
    const cf* twN = nullptr;              // exp(-2 pi i k / n_fft), k <= M
    const float* window = nullptr;        // [n_fft] periodic window of win_length samples, zero-padded and centred
    const float* window2 = nullptr;       // its square
    const float* env = nullptr;           // overlap-add envelope: head [n_fft], interior [hop], tail [n_fft/2]
};

// Overlap-add envelope sum_t w^2[p - hop t] at padded position p of a clip of T frames, frames in ascending order.
AW_HD float gen_env_loop(const float* w2, int N, int hop, int p, int T) {
    const int tlo = p - N + 1 > 0 ? (p - N + hop) / hop : 0;
    const int thi = (p / hop < T - 1) ? p / hop : T - 1;
    float e = 0.f;
    for (int t = tlo; t <= thi; ++t) e += w2[p - hop * t];
    return e;
}
// The same value from the plan's tables (built with gen_env_loop): with T*hop >= N the envelope depends only on p
// below N (head), on p mod hop in between (interior), and on p - T*hop from T*hop on (tail).
AW_HD float gen_env(const float* env, const float* w2, int N, int hop, int p, int T) {
    if ((long)T * hop < N) return gen_env_loop(w2, N, hop, p, T);
    if (p < N) return env[p];
    const int q = p - T * hop;
    if (q >= 0) return env[N + hop + (q < N / 2 ? q : N / 2 - 1)];
    return env[N + p % hop];
}

struct GenLaunch {
    GenPlanDev plan;
    int B = 0, NF = 0, max_len = 0;
    const int* frame_off = nullptr;       // [B+1]
    const int* sig_off = nullptr;         // clip signals (aware_stft input, aware_stft_bwd output)
    const int* sig_len = nullptr;
    const int* out_off = nullptr;         // istft-length signals (aware_istft output, aware_istft_bwd input)
    const int* out_len = nullptr;
    const unsigned long long* pmax = nullptr;   // per-clip |x| partial maxima (normalisation) or null
    const int* pcount = nullptr;
    int pstride = 0;
    float* frames = nullptr;              // [NF][n_fft] windowed frames between the transform and the overlap-add
};
// analysis: frames -> window -> rFFT -> spectrum rows.  adjoint = 0: aware_stft (reflect pads, optional normaliser);
// 1: aware_istft_bwd (the trimmed gradient over the envelope, irfft's adjoint weights on the bins)
void launch_gen_analysis(const GenLaunch& L, const float* sig, void* spec, int adjoint, hipStream_t st);
// synthesis: spectrum rows -> irFFT -> window -> L.frames, then overlap-add.  adjoint = 0: aware_istft (divide by the
// envelope, trim); 1: aware_stft_bwd (no envelope, reflect pads folded back in)
void launch_gen_synthesis(const GenLaunch& L, const void* spec, float* out, int adjoint, hipStream_t st);
// out /= max|out| + 1e-8 per clip over the istft-length signals (L.pmax: partials of `out`)
void launch_gen_normalize(const GenLaunch& L, float* out, hipStream_t st);

// ---- loop_any.hip: the band kernels of the embed / detect loop on a general plan -------------------------------------
// Rows of the general spectrum (`sstride` complex values, bins 0..n_fft/2) on one side, band rows in the detector's layout
// (`bstride` floats, column f = bin band_lo + f, columns nband..bstride-1 padding) on the other; NF rows, ragged over
// frame_off.  Threads exist for the band columns only.
struct BandLaunch {
    int NF = 0, B = 0;
    const int* frame_off = nullptr;       // [B+1]
    int sstride = 0;                      // GenPlanDev::stride
    int band_lo = 0, nband = 0, bstride = 0;
};
// what band_mag also writes at aware_embed_begin: the unit phasors of the original spectrum, the coefficients, their box
// (box_bounds, the card route's formula) and the optimiser state
struct BandBegin {
    void* unit = nullptr;                 // cf [NF][bstride], (1, 0) where |S| == 0, (0, 0) in the padding
    float *coef = nullptr, *lo = nullptr, *hi = nullptr, *mom = nullptr, *vel = nullptr, *best = nullptr, *c0 = nullptr;
    float ratio = 0.f;                    // 10^(-tolerance_db / 20)
};
// mag[row][f] = |spec[row][band_lo + f]|, padding columns zero; begin != null: the arrays of BandBegin too.  exact (always
// with begin): by polar_exact (polar.hpp), for spectra of the original audio; false: the plain form of the loop's launch
void launch_band_mag(const BandLaunch& L, const void* spec, float* mag, const BandBegin* begin, bool exact, hipStream_t st);
// spec[row][band_lo + f] = coef[row][f] * unit[row][f]; every other bin of spec is left as it is
void launch_band_assemble(const BandLaunch& L, const float* coef, const void* unit, void* spec, hipStream_t st);
// gspec[row][band_lo + f] = gmag[row][f] * spec / |spec| (0 where |spec| == 0); every other bin of gspec is left as it is
// (the caller zeroed it once)
void launch_band_mag_bwd(const BandLaunch& L, const void* spec, const float* gmag, void* gspec, hipStream_t st);
// g[row][f] = Re(conj(unit[row][f]) * gspec[row][band_lo + f]) -> grad_out (may be null); do_step: the model card's NAdam
// step, the clamp to the box and the best snapshot of the clips in `improved`, as the card route's analysis adjoint does
// them (nadam_clamp_update with sched[*step - 1])
struct BandStep {
    float *coef = nullptr, *mom = nullptr, *vel = nullptr, *best = nullptr;
    const float *lo = nullptr, *hi = nullptr;
    const int* improved = nullptr;        // [B]
    const void* sched = nullptr;          // float4 per step {c_grad, c_mom, bias_correction2, 0}
    int sched_len = 0;
    const int* step = nullptr;            // device step counter (already advanced by the read-out)
    float hyp[4] = {0.f, 0.f, 0.f, 0.f};  // {1 - beta1, beta2, 1 - beta2, eps}
};
// out[off[b] + i] = rescale[b] * (in[off[b] + i] / (max|in_b| + 1e-8)) (rescale null: 1): the last normaliser of an embed run and
// the caller's rescale, on ragged signals (pmax: partial maxima of `in`)
void launch_rescale_normalize(const float* in, float* out, const int* off, const int* len, const unsigned long long* pmax,
                              const int* pcount, int pstride, const float* rescale, int B, int max_len, hipStream_t st);
void launch_band_coef_grad(const BandLaunch& L, const void* gspec, const void* unit, float* grad_out, const BandStep* step,
                           hipStream_t st);

// ---- loop_any_chain.hip: attack-aware embedding on the general route (EXTENSION, aware_embed_set_general_chain): the
// element-wise kinds of a chain between the general loop's synthesis and its analysis, on pieces of kGenChainPiece samples
// (loop_any_chain.hpp) of signals at any float offset -------------------------------------------------------------------
struct GenChainLaunch {
    const int* sig_off = nullptr;         // [B] out_off: any float offset
    const int* sig_len = nullptr;         // [B] Ny_b
    const int* pc_out = nullptr;          // [B] 4096-sample pieces of clip b: the partials of pmaxY
    int B = 0, pstride = 0;               // pstride: stride of pmaxY
    int pieces = 0;                       // pieces of the longest clip: the grid, and the stride of the chain's partial arrays
    const int* step = nullptr;            // device step counter; step_back = 1 once the read-out kernel has advanced it
    int step_back = 0;
    const unsigned* seeds = nullptr;      // [B]
    int n = 0;
    int kind[kMaxLoopAttacks] = {0};
    int k[kMaxLoopAttacks] = {0};
    double inv_snr[kMaxLoopAttacks] = {0};
    float prob[kMaxLoopAttacks] = {0};
    int p_lo[kMaxLoopAttacks] = {0}, p_hi[kMaxLoopAttacks] = {0};
    float floor[kMaxLoopAttacks] = {0};
    const float* yraw = nullptr;          // the raw synthesis and its partial maxima (4096-sample pieces)
    const unsigned long long* pmaxY = nullptr;
    double* psq = nullptr;                // [kMaxLoopAttacks][B][pieces]
    float* z = nullptr;                   // the attacked signal and its partial maxima
    unsigned long long* pmaxZ = nullptr;  // [B][pieces]
    float* a = nullptr;                   // N(N(z)): what the loop's analysis reads
    float* gy = nullptr;                  // backward: dL/da in, dL/dyraw out
    double* pdotA = nullptr;              // [B][pieces] partial sums of dL/da * a
    double* pdotX = nullptr;              // [B][pieces] partial sums of dL/dx * x
};
// x = N(N(yraw)), the chain, z and its partial maxima, a = N(N(z)): one reduction launch per noise entry, then two passes
void launch_gen_chain_forward(const GenChainLaunch& L, hipStream_t st);
// gy: dL/da -> dL/dyraw in place, in three passes: the partial sums of dL/da * a; the normalisers at z and the chain's masks
// and gains with the partial sums of dL/dx * x; the normalisers in front of the chain
void launch_gen_chain_backward(const GenChainLaunch& L, hipStream_t st);

// ---- stoi_kernels.hip: batched short-time objective intelligibility (metrics/audio.py::stoi) at 10 kHz -------------
constexpr int kStoiFrame = 256, kStoiHop = 128, kStoiBands = 15, kStoiRow = 16, kStoiN = 30;
constexpr int kStoiSegChunk = 64;         // segments per partial sum of the last stage
// first-stage frames of a clip of n samples: len(range(0, n - 256, 128)) -- a frame that would end at n is not taken
AW_HD int stoi_frames(int n) { return n > kStoiFrame ? (n - kStoiFrame + kStoiHop - 1) / kStoiHop : 0; }
// partial sums per clip of the segment stage for a clip of n samples (every frame kept)
AW_HD int stoi_partials(int n) {
    const int nseg = stoi_frames(n) - 1 - (kStoiN - 1);
    return nseg > 0 ? (nseg + kStoiSegChunk - 1) / kStoiSegChunk : 1;
}
struct StoiTables {
    const cf* th = nullptr;               // W_256^j, j < 128
    const cf* twN = nullptr;              // exp(-2 pi i k / 512), k <= 256
    const float* window = nullptr;        // np.hanning(258)[1:-1]
    const int* bands = nullptr;           // lo[16] then hi[16]: bins [lo, hi) of third-octave band j < 15; entry 15 is empty
};
struct StoiLaunch {
    StoiTables tab;
    const float* clean = nullptr; const int* clean_off = nullptr;
    const float* proc = nullptr; const int* proc_off = nullptr;
    const int* n = nullptr;               // [B] common length of clip b in both signals
    int B = 0, max_frames = 0, max_partials = 0;
    double* energy = nullptr;             // [total frames] frame energies of the clean signal, dB
    int* kept = nullptr;                  // [total frames] clip b's kept frames, ascending, from fbase[b]
    int* kcount = nullptr;                // [B] kept frames K_b
    int* fbase = nullptr;                 // [B] first row of clip b in energy / kept / xt / yt
    float* xt = nullptr; float* yt = nullptr;   // [total frames][16] third-octave band magnitudes of the re-framed signals
    double* partial = nullptr;            // [B][max_partials]
    double* out = nullptr;                // [B]
    int* kept_out = nullptr;              // [B] or null
};
void launch_stoi(const StoiLaunch& L, hipStream_t st);

// ---- loop_attack_kernels.hip: attack-aware embedding (EXTENSION): a chain of attacks between the embed loop's synthesis and
// its analysis, drawn afresh at every optimiser step (aware_embed_set_loop_attacks) --------------------------------------
struct LoopAttackLaunch {
    const int* frame_off = nullptr;
    const int* pcount = nullptr;          // [B] synthesis runs per clip: the partials' layout
    int B = 0, pstride = 0, run_blocks = 0;
    const int* step = nullptr;            // device step counter; step_back = 1 once the read-out kernel has advanced it
    int step_back = 0;
    const unsigned* seeds = nullptr;      // [B]
    int n = 0;
    int kind[kMaxLoopAttacks] = {0};
    int k[kMaxLoopAttacks] = {0};         // suppression: samples
    double inv_snr[kMaxLoopAttacks] = {0};   // noise: 10^(-snr_db / 10)
    float prob[kMaxLoopAttacks] = {0};
    int p_lo[kMaxLoopAttacks] = {0}, p_hi[kMaxLoopAttacks] = {0};      // gain envelope: samples between breakpoints
    float floor[kMaxLoopAttacks] = {0};   // gain envelope: the lowest gain
    const float* yraw = nullptr;          // the raw synthesis and its partial maxima
    const unsigned long long* pmaxY = nullptr;
    double* psq = nullptr;                // [kMaxLoopAttacks][B][pstride]
    float* z = nullptr;                   // the attacked signal (layout of yraw) and its partial maxima
    unsigned long long* pmaxZ = nullptr;
    float* gy = nullptr;                  // backward: gradient in / out
    float* gy_out = nullptr;              // backward: where a stage writes instead of gy (null: in place)
    const float* gpad = nullptr;          // reflect-pad parts of the streaming synthesis adjoint (null: already folded)
    const double* pdot_in = nullptr;
    double* pdot_out = nullptr;
    // chains with a splitting entry (loop_chain.hpp) or a gain envelope: a clip on which no entry fires at a step leaves the plain loop's
    // bits (its maxima are recorded as 1, the backward stages pass gradient, partial sums and reflect pads through);
    // gpad_out: [B][2][512], the pads the analysis adjoint then reads (zeros for every other clip)
    int idle_plain = 0;
    float* gpad_out = nullptr;
    LoopGate gate;                        // inside a mixture: the clips that drew this chain
};
// x = N(N(yraw)), the chain, z and the partial maxima of |z|: one reduction launch per noise entry, then one pass
void launch_loop_attack_forward(const LoopAttackLaunch& L, hipStream_t st);
// gy: dL/d N(N(z)) -> dL/dx in place, pdot_out: partial sums of dL/dx * x
void launch_loop_attack_backward(const LoopAttackLaunch& L, hipStream_t st);
// the same in stages, for a chain that a reverberation or a speed change splits: entries [j0, j1) on src (norm 1: src is the raw synthesis and
// x = N(N(src)); 0: src is x itself) -> dst (may be src) and, unless null, the partial maxima of |dst|
void launch_loop_attack_stage(const LoopAttackLaunch& L, int j0, int j1, const float* src, int norm, float* dst,
                              unsigned long long* pmax, hipStream_t st);
// backward of entries [j0, j1) on gy in place (into gy_out when set; an idle clip is then copied); at_z: the normalisers' backward at z and the reflect pads come first;
// dot: the partial sums of the result against x go to pdot_out
void launch_loop_attack_stage_bwd(const LoopAttackLaunch& L, int j0, int j1, int at_z, int dot, hipStream_t st);

// The loop side of a stage kernel that serves one splitting entry of a chain (kinds 3 to 7): the embed loop's layout (x and z
// both Ny_b long at sig_offset, one workgroup per synthesis run) and the entry's draw (loop_rng.hpp loop_entry_draw)
struct LoopDraw {
    const int* frame_off = nullptr;       // [B + 1]
    int pstride = 0, run_blocks = 0;
    const int* step = nullptr; int step_back = 0;      // device step counter; step_back = 1 once the read-out kernel has advanced it
    const unsigned* seeds = nullptr;      // [B]
    int entry = 0;
    float prob = 0.f;
    LoopGate gate;                        // inside a mixture: the clips that drew this chain
};
// the grid of a stage kernel: in the loop one workgroup per synthesis run and clip, stand-alone one per `per_wg` samples of the
// longest clip (max_len) and clip
inline dim3 stage_grid(const LoopDraw& d, int B, int max_len, int per_wg) {
    return dim3(d.frame_off ? (unsigned)d.pstride : (unsigned)((max_len + per_wg - 1) / per_wg), (unsigned)B, 1);
}

// ---- loop_reverb_kernels.hip: reverberation (EXTENSION): a drawn impulse response per clip and the partitioned FFT
// convolution that applies it, inside the embed loop (chain kind 2) and stand-alone (aware_convolve, aware_reverb_ir) ----
struct ReverbIrLaunch {
    const unsigned* seeds = nullptr;      // [B]
    const int* step = nullptr;            // device step counter, or null: step_imm
    int step_imm = 0, entry = 0, B = 0;
    int n_lo = 0, n_hi = 0;               // taps, drawn uniformly in [n_lo, n_hi]
    double gain = 0;                      // 10^(drr_db / 20)
    float prob = 1.f;
    float* h = nullptr; int h_stride = 0; // [B][h_stride], zero beyond the drawn length
    int* nh = nullptr;                    // [B] the drawn length; 0: the entry does not fire (h is then the unit impulse)
    LoopGate gate;
};
void launch_reverb_ir(const ReverbIrLaunch& L, hipStream_t st);
struct ConvolveLaunch {
    const cf* tables = nullptr;           // kReverbTwHalf + kReverbBins values
    const float* in = nullptr; float* out = nullptr;     // out may be in
    const int* off = nullptr; const int* len = nullptr;  // [B] float offset and length of clip b, or
    const int* frame_off = nullptr;       // the embed loop's layout (common.hpp sig_offset), when off is null
    int B = 0, kmax = 0;                  // kmax >= blocks of the longest clip
    const float* h = nullptr; int h_stride = 0; const int* nh = nullptr;
    int parts = kReverbParts;             // partitions hspec has room for
    int adjoint = 0;                      // 0: out = (h * in)[0 : len]; 1: out[i] = sum_k h[k] in[i + k]
    int skip_h = 0;                       // hspec is that of an earlier launch with the same h
    cf* hspec = nullptr;                  // [B][parts][kReverbBins]
    cf* xspec = nullptr;                  // [B][kmax][kReverbBins]
    LoopGate gate;
};
void launch_convolve(const ConvolveLaunch& L, hipStream_t st);

// ---- loop_speed_kernels.hip, loop_stretch_kernels.hip, loop_pitch_kernels.hip: the in -> out resamplers (EXTENSION), inside
// the embed loop and stand-alone, each with its adjoint in gather form.  Speed change (chain kind 3, aware_speed_change):
// Catmull-Rom resampling at a drawn ratio R / 65536.  Time stretch (kind 4, aware_stretch_ola): overlap-add of Hann-windowed
// segments taken at a drawn rate Q / 65536.  Pitch shift (kind 5, aware_pitch_shift_ola): the speed change at R / 65536 of the
// stretch at the coupled rate Q = round(2^32 / R), fused (the stretched signal lives in LDS only) ------------------------------
constexpr int kResampleThreads = 256;     // every thread owns four consecutive outputs
struct ResampleLaunch {
    const float* in = nullptr; float* out = nullptr;      // never the same buffer
    const float* window = nullptr;        // stretch_window(); not read by the speed change
    int B = 0, adjoint = 0;               // 0: out = z from in = x; 1: out = gx from in = gz
    // the embed loop (draw.frame_off set): m drawn in the kernel
    LoopDraw draw;
    int m_lo = 0, m_hi = 0;               // the pitch shift's are speed offsets, inside kSpeedMin .. kSpeedMax
    int coin = 0;                         // read by the speed change only.  1: behind a phase vocoder with both modes, m = 0 where the draw's r[2] < 2^31 (stretch mode)
    // or a ragged batch (draw.frame_off null): x is x_len[b] floats at x_off[b], z is z_len[b] floats at z_off[b], m[b] given
    const int* x_off = nullptr; const int* x_len = nullptr;
    const int* z_off = nullptr; const int* z_len = nullptr;
    int max_len = 0;                      // >= every length written
    const int* m = nullptr;               // [B]
};
// the periodic Hann window of 1024 points in f32 on the current device (uploaded once, outside any stream capture); null
// when the device refuses
const float* stretch_window();
void launch_speed_change(const ResampleLaunch& L, hipStream_t st);
void launch_time_stretch(const ResampleLaunch& L, hipStream_t st);
void launch_pitch_shift(const ResampleLaunch& L, hipStream_t st);

// ---- loop_pv_kernels.hip: phase vocoder on the frames of a spectrum (EXTENSION): magnitudes interpolated at the rate
// Q / 65536, phases accumulated as a product of unit phasors, inside the embed loop (chain kind 6, between the staged STFT and
// iSTFT) and stand-alone (aware_pv_frames, aware_pv_frames_bwd) -------------------------------------------------------------
struct PvLaunch {
    const void* spec = nullptr;           // S [NF][520] complex
    const void* grad = nullptr;           // backward: G = dL/dY [NF][520]; never `out`
    void* out = nullptr;                  // forward: Y; backward: gS (may be `spec`)
    int B = 0;
    // draw.frame_off [B + 1] always; the embed loop (draw.seeds non-null): the mode and the offset drawn in the kernel; a clip
    // that the entry leaves alone is skipped
    LoopDraw draw;
    int q_lo = 0, q_hi = -1;              // stretch offsets, inside kStretchMin .. kStretchMax; lo > hi: no stretch mode
    int m_lo = 0, m_hi = -1;              // speed offsets, inside kSpeedMin .. kSpeedMax; lo > hi: no pitch mode
    // or stand-alone (draw.seeds null): mq[b] given, outside kStretchMin .. kStretchMax read as 0 (the identity)
    const int* mq = nullptr;              // [B]
};
void launch_pv_frames(const PvLaunch& L, int backward, hipStream_t st);
// the loop's clips that the entry leaves alone at this step: dst = src (the embed loop's signal layout)
void launch_pv_idle(const PvLaunch& L, const float* src, float* dst, hipStream_t st);

// ---- loop_delete_kernels.hip: sample deletion (EXTENSION): k samples cut out at `start`, the remainder moved up, zeros at the
// end, inside the embed loop (chain kind 7) and stand-alone (aware_delete_samples), and its adjoint in gather form ---------
struct DeleteLaunch {
    const float* in = nullptr; float* out = nullptr;      // never the same buffer
    int B = 0, adjoint = 0;               // 0: out = z from in = x; 1: out = gx from in = gz
    // the embed loop (draw.frame_off set): start and k drawn in the kernel
    LoopDraw draw;
    int k_lo = 0, k_hi = 0;    // 1 <= k_lo <= k_hi < every Ny_b
    int at = 0;                           // 0: the cut starts at sample 0; 1: anywhere
    // or a ragged batch (draw.frame_off null): both sides are len[b] floats at off[b]; start[b] and k[b] given, clamped to the clip
    const int* off = nullptr; const int* len = nullptr;
    int max_len = 0;                      // >= every length
    const int* start = nullptr;           // [B]
    const int* k = nullptr;               // [B]
};
void launch_delete_samples(const DeleteLaunch& L, hipStream_t st);

// ---- loop_gain_kernels.hip: gain envelope (EXTENSION): the element-wise chain kind 8 alone (aware_gain_envelope); inside the
// embed loop it runs in the stage kernels of loop_attack_kernels.hip (loop_gain.hpp holds what the two share) ---------------
struct GainLaunch {
    const float* in = nullptr; float* out = nullptr;      // may be the same buffer
    float* gains = nullptr;               // null, or the layout of out: g itself
    const int* off = nullptr; const int* len = nullptr;   // [B] float offset and length of clip b
    int B = 0, max_len = 0;               // max_len >= every length
    const unsigned* seeds = nullptr;      // [B]
    int step = 0, entry = 0;
    int p_lo = 0, p_hi = 0;               // kEnvelopeMinPeriod <= p_lo <= p_hi <= kEnvelopeMaxPeriod
    float floor = 0.f;
};
void launch_gain_envelope(const GainLaunch& L, hipStream_t st);

// ---- loop_filter_kernels.hip: band filter (EXTENSION): a zero-phase windowed-sinc FIR of 2 kFilterHalf + 1 taps, low-pass,
// high-pass, band-pass or band-stop at edges in units of 1 / 65536 cycle per sample, inside the embed loop (chain kind 9) and
// stand-alone (aware_band_filter).  Its own adjoint: the backward pass is the same launch on the gradient -------------------
struct FilterLaunch {
    const float* in = nullptr; float* out = nullptr;      // never the same buffer
    int B = 0, adjoint = 0;               // adjoint is not read: h is symmetric and the extension is by zeros
    // the embed loop (draw.frame_off set): the response and the edges drawn in the kernel
    LoopDraw draw;
    int mask = 0;                         // bits 1 lowpass, 2 highpass, 4 bandpass, 8 bandstop: the responses drawn from
    int c_lo = 0, c_hi = 0, w_min = 0;    // 1 <= c_lo <= c_hi, 1 <= w_min, c_hi + w_min <= kFilterMaxEdge
    // or a ragged batch (draw.frame_off null): both sides are len[b] floats at off[b]; response[b] (one bit), c1[b], c2[b] given
    const int* off = nullptr; const int* len = nullptr;
    int max_len = 0;                      // >= every length
    const int* response = nullptr;        // [B]
    const int* c1 = nullptr;              // [B]
    const int* c2 = nullptr;              // [B] read by the band responses
    float* taps = nullptr;                // null, or [B][256]: tap k at index k + kFilterHalf, zero at 255
};
void launch_band_filter(const FilterLaunch& L, hipStream_t st);

// ---- loop_shift_kernels.hip: frequency shift (EXTENSION): single-sideband modulation, z = x cos phi - (Hx) sin phi with H a
// Hilbert transformer of 2 kFilterHalf + 1 taps and phi_i = 2 pi ((p0 + i d) mod 2^20) / 2^20, inside the embed loop (chain
// kind 12) and stand-alone (aware_frequency_shift), and its exact adjoint gx = g cos phi + H(g sin phi) ------------------------
struct ShiftLaunch {
    const float* in = nullptr; float* out = nullptr;      // never the same buffer
    int B = 0, adjoint = 0;               // 0: out = z from in = x; 1: out = gx from in = gz
    // the embed loop (draw.frame_off set): d and p0 drawn in the kernel
    LoopDraw draw;
    int d_lo = 0, d_hi = 0;               // -kShiftMax <= d_lo <= d_hi <= kShiftMax, in units of sr / 2^20 Hz
    // or a ragged batch (draw.frame_off null): both sides are len[b] floats at off[b]; d[b] and p0[b] given
    const int* off = nullptr; const int* len = nullptr;
    int max_len = 0;                      // >= every length
    const int* d = nullptr;               // [B]
    const int* p0 = nullptr;              // [B] read modulo 2^20
};
void launch_frequency_shift(const ShiftLaunch& L, hipStream_t st);

// ---- loop_excerpt_kernels.hip: tiled excerpt (EXTENSION): the excerpt [start, start + L) of the clip repeated periodically
// until it fills the clip, inside the embed loop (chain kind 10) and stand-alone (aware_excerpt_tile), and its adjoint in
// gather form: the sum over the periods in f32, m ascending ------------------------------------------------------------------
struct ExcerptLaunch {
    const float* in = nullptr; float* out = nullptr;      // never the same buffer
    int B = 0, adjoint = 0;               // 0: out = z from in = x; 1: out = gx from in = gz
    // the embed loop (draw.frame_off set): start and L drawn in the kernel
    LoopDraw draw;
    int l_lo = 0, l_hi = 0;               // kExcerptMinLen <= l_lo <= l_hi; a draw above Ny_b is read as Ny_b
    // or a ragged batch (draw.frame_off null): both sides are len[b] floats at off[b]; start[b] and length[b] given, clamped to the clip
    const int* off = nullptr; const int* len = nullptr;
    int max_len = 0;                      // >= every length
    const int* start = nullptr;           // [B]
    const int* length = nullptr;          // [B]
};
void launch_excerpt_tile(const ExcerptLaunch& L, hipStream_t st);

// ---- loop_warp_kernels.hip: time warp (EXTENSION): the clip resampled through the speed change's Catmull-Rom taps at a rate
// that is piecewise linear in time between breakpoints 2^e samples apart, every position exact in 64-bit integers, inside the
// embed loop (chain kind 11) and stand-alone (aware_time_warp), and its adjoint in gather form.  The forward launch fills the
// table (R_k, A(k)) first; the adjoint launch reads it ------------------------------------------------------------------------
struct WarpLaunch {
    const float* in = nullptr; float* out = nullptr;      // never the same buffer
    int B = 0, adjoint = 0;               // 0: out = z from in = x; 1: out = gx from in = gz
    int* table_r = nullptr;               // [B][stride] R_k = 65536 + m_k
    long long* table_a = nullptr;         // [B][stride] A(k)
    int stride = 0;                       // >= warp_breakpoints(Ny_b, e) of every clip; an index from `stride` on reads the last entry
    // the embed loop (draw.frame_off set): e, ph and the m_k drawn in the kernels
    LoopDraw draw;
    int e_lo = 0, e_hi = 0, depth = 0;    // kWarpMinExp <= e_lo <= e_hi <= kWarpMaxExp, 1 <= depth <= kWarpMaxDepth
    // or a ragged batch (draw.frame_off null): both sides are len[b] floats at off[b]; e[b], ph[b] and the m_k given, clamped
    const int* off = nullptr; const int* len = nullptr;
    int max_len = 0;                      // >= every length
    const int* e = nullptr;               // [B]
    const int* ph = nullptr;              // [B]
    const int* rates = nullptr;           // [B][stride] m_k
};
void launch_time_warp(const WarpLaunch& L, hipStream_t st);

// ---- sync_kernels.hip: offset search in detection (EXTENSION): values [B][n][L] -> the row of the largest mean |v - centre|
// per clip (the smallest j on a tie), its index and that mean; one wave per clip ------------------------------------------
void launch_sync_select(const float* values, int B, int n, int L, float centre, float* out_values, int* out_index,
                        float* out_conf, hipStream_t st);

// ---- speed_search_kernels.hip: speed search in detection (EXTENSION): every clip of a ragged batch resampled at n_views
// speed offsets m[j] in one launch; view (b, j) is ((in_len[b] - 1) << 16) / (65536 + m[j]) + 1 floats at
// out_off[b * n_views + j], bit for bit what launch_speed_change gives at that m and length ---------------------------------
void launch_speed_views(const float* in, const int* in_off, const int* in_len, int B, const int* m, int n_views, float* out,
                        const int* out_off, int max_len, hipStream_t st);

// ---- shift_search_kernels.hip: shift search in detection (EXTENSION): every clip of a ragged batch moved by n_views
// frequency shifts d[j] (units of sr / 2^20 Hz, |d| <= kShiftMax, start phase 0) in one launch; view (b, j) is in_len[b]
// floats at out_off[b * n_views + j], bit for bit what launch_frequency_shift gives at that d and p0 = 0 ---------------------
void launch_shift_views(const float* in, const int* in_off, const int* in_len, int B, const int* d, int n_views, float* out,
                        const int* out_off, int max_len, hipStream_t st);

// ---- scan_kernels.hip: scanning long recordings (EXTENSION).  launch_scan_select: values [W][n][L] -> per window the
// confidence, index, row and packed decision bits ([W][ceil(L / 32)]) of the most confident view; one wave per window.
// launch_scan_segments: per file b (windows win_off[b] .. win_off[b + 1], dev int [B + 1]) the runs of marked windows that
// agree on their bits; one workgroup per file; the seg_* arrays are [B][max_segments], slots beyond a file's runs untouched
constexpr int kScanMaxBits = 512;      // L of both kernels: a lane of scan_segments_kernel keeps 512 / 64 sums in registers
void launch_scan_select(const float* values, int W, int n, int L, float centre, float* win_conf, int* win_view,
                        float* win_values, unsigned* win_bits, hipStream_t st);
struct ScanSegments {
    const float* win_conf = nullptr; const int* win_view = nullptr; const float* win_values = nullptr;
    const unsigned* win_bits = nullptr; const int* win_off = nullptr;
    int B = 0, L = 0, max_flip = 0, max_segments = 0;
    float centre = 0.f, min_conf = 0.f;
    int* n_seg = nullptr; int* seg_first = nullptr; int* seg_last = nullptr; int* seg_peak = nullptr; int* seg_view = nullptr;
    float* seg_conf = nullptr; float* seg_values = nullptr;
};
void launch_scan_segments(const ScanSegments& S, hipStream_t st);

// ---- viterbi_kernels.hip: coded payloads (EXTENSION).  values [R][L] -> per row the T = L / n decoded input bits packed
// into ceil(T / 32) words, the final path metric, the CRC's verdict and the count of corrected positions; one wave per row
constexpr int kViterbiMaxBits = 512;   // L: T <= 256 steps, four survivor registers per lane
constexpr int kViterbiMaxRows = 1 << 20;
constexpr int kViterbiRows = 4;        // rows (waves) per workgroup
void launch_viterbi(const float* values, int R, int L, float centre, int n, int c, unsigned* bits, float* metric, int* valid,
                    int* corrected, hipStream_t st);

}  // namespace aware
