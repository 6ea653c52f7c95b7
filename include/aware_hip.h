/* libaware_hip -- C ABI of the MI355X (gfx950) AWARE hot path.
 *
 * The drop-in boundary for deepmarkpy/aware's embed -> attack -> detect path.  The
 * reference has no FFI of its own (it is pure Python); the seam it offers is the
 * plugin call  BaseAudioProcessor.__call__(tensor) -> tensor
 * (src/AWARE/interfaces/audio.py:6-9) plus AWAREEmbedder.embed / AWAREDetector.detect
 * (src/AWARE/interfaces/embedding.py:5-8, interfaces/detection.py:6-14) and
 * Attack.apply(audio, sr) (scripts/attacks.py:16-30).  Each entry point below names
 * the reference code it replaces.  The host side (aware_amd/, Python + ctypes) maps
 * these onto the reference's class / function names; see INTEGRATION.md.
 *
 * Conventions
 *   - every pointer marked "dev" is a device (HBM) pointer owned by the caller
 *     (PyTorch-ROCm tensors' data_ptr()); the library never frees caller memory;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     all work is enqueued on it, no entry point synchronises unless documented;
 *   - return value: 0 on success, a negative AWARE_E_* code otherwise; nothing throws;
 *   - all arithmetic is IEEE fp32 unless a parameter says f64;
 *   - a "batch" is a ragged set of B mono clips; clip b has n_b samples,
 *     T_b = 1 + n_b/256 frames, Ny_b = 256*(T_b-1) output samples, T_b/2 pooled frames.
 *   - band-limited spectra are frame-major [total frames][aware_plan_band_stride(plan)] (column f
 *     is bin band_lo + f; the model card's band: 225 columns, bins 32..256 = 500..4000 Hz at 16 kHz,
 *     n_fft 1024, of 256; the tail is zero).  The stride is AWARE_SPEC_STRIDE = 256 for a band
 *     inside bins 1..511 at most 256 bins wide (the narrow layout), AWARE_SPEC_STRIDE_WIDE = 576
 *     for any other band inside bins 0..512 (the wide layout).  Every band-limited array of this
 *     header -- aware_stft_band's mag / phasor, aware_detector_forward / _backward's mag /
 *     grad_mag, aware_embed_gradient's grad and the embed views -- has that many floats per row.
 */
#ifndef AWARE_HIP_H
#define AWARE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AWARE_OK 0
#define AWARE_E_BADARG (-1)
#define AWARE_E_UNSUPPORTED (-2)   /* e.g. n_fft outside {256, ..., 4096}, a general plan where only the card's geometry runs (loop attacks, the L1 loss) */
#define AWARE_E_HIP (-3)           /* a HIP runtime call failed; see aware_last_hip_error() */
#define AWARE_E_WORKSPACE (-4)     /* caller's workspace too small */

/* loss kinds (embedding/losses.py:95-103 and two additions) */
#define AWARE_LOSS_PUSH_EXTREMES 0
#define AWARE_LOSS_MSE 1
#define AWARE_LOSS_HINGE 2
#define AWARE_LOSS_SIGN 3
#define AWARE_LOSS_PUSH_SIGMOID 4
#define AWARE_LOSS_BER 5            /* no gradient, losses.py:90-92 */
#define AWARE_LOSS_PUSH_L1 6        /* EXTENSION (BASELINE config 3 "BER+L1"): push_extremes + l1_weight * mean|c - c0| */
#define AWARE_LOSS_EXTERNAL 7       /* internal: `target` holds dL/dpred (aware_detector_backward) */
#define AWARE_LOSS_BCE 8            /* losses.py:79-81, torch's binary_cross_entropy: targets 0 / 1; detectors whose final
                                       activation is AWARE_FINAL_SIGMOID only (aware_embed_create: AWARE_E_UNSUPPORTED otherwise) */

#define AWARE_SPEC_STRIDE 256      /* floats per frame row of a band-limited array (narrow layout) */
#define AWARE_SPEC_STRIDE_WIDE 576 /* ... of a band with the wide layout (aware_plan_band_stride) */
#define AWARE_FULL_STRIDE 520      /* complex values per frame row of a full one-sided spectrum */

typedef struct aware_plan aware_plan;
typedef struct aware_detector aware_detector;
typedef struct aware_batch aware_batch;
typedef struct aware_embed aware_embed;
typedef struct aware_stoi_plan aware_stoi_plan;

/* ABI version (200: no process-global knobs, the kernel choices live in aware_embed_config; 300: conv_pipe 0 = f16 two-term
 * kernels, optimiser / scheduler registries, device-side detector training, aware_stft_bwd for any clip length; 310: general
 * STFT geometry -- aware_plan_create_ex, aware_plan_spectrum_stride, aware_plan_is_general, aware_batch_create_for_plan,
 * aware_nola_check; 320: detector architecture variants -- aware_detector_create_ex, aware_detector_is_card; 330: any
 * embedding band inside bins 0..512 -- the wide layout, aware_plan_band_stride; 340: payloads of 1..512 bits --
 * aware_detector_create accepts any even channels[n_layers] from 2 to 1024; 350: detector sizes -- n_mels 1..512, hidden
 * widths 1..4096, n_layers 1..33).  The STOI entry points (aware_stoi_create, aware_stoi_destroy, aware_stoi_workspace_bytes,
 * aware_stoi, aware_stoi_band_edges, aware_stoi_frames) were added without a version step -- tests/test_detector_sizes_host.py
 * pins the literal 350 -- so a caller detects them by symbol.  The embed / detect loop on general plans (the general route)
 * came without a version step for the same reason and adds no symbol: a caller detects it by aware_detector_create
 * returning AWARE_OK for a plan created with AWARE_PLAN_GENERAL (before: AWARE_E_UNSUPPORTED). */
int aware_version(void);
/* text of the last failed HIP runtime call on the calling thread (thread-local) */
const char* aware_last_hip_error(void);
/* The library keeps no mutable process-global state: handles are independent, every entry point may be called
 * from any host thread on any stream (one thread at a time per handle).  The only shared object is a mutex-guarded
 * memo of measured GEMM tile choices, which never changes a result (all tile configurations are bit-identical). */

/* ---- plan: FFT twiddles, window, band ------------------------------------------------
 * Replaces the constructor state of STFT / ISTFT (src/AWARE/utils/audio/stft.py:14-25,
 * :34-45: n_fft, hop_length, window "hann"|"hamming", win_length) and
 * AWAREEmbedder._get_embedding_frequency_indices (embedding/multibit_embedder.py:43-47).
 * window: 0 = hann (periodic), 1 = hamming (periodic).  band_lo_bin/band_hi_bin inclusive, any band with
 * 0 <= band_lo_bin <= band_hi_bin <= n_fft/2 (else AWARE_E_UNSUPPORTED); aware_plan_band_stride gives its row layout. */
int aware_plan_create(aware_plan** out, int n_fft, int hop, int win_length, int window,
                      int band_lo_bin, int band_hi_bin);
void aware_plan_destroy(aware_plan* plan);
/* Geometries.  The model card's (n_fft 1024, hop 256, win_length 1024) gives a card plan: the kernels of the embed / detect
 * loop.  Every other geometry with n_fft in {256, 512, 1024, 2048, 4096} (else AWARE_E_UNSUPPORTED), 1 <= hop <= n_fft and
 * 1 <= win_length <= n_fft (else AWARE_E_BADARG) gives a GENERAL plan (csrc/stft_any.hip): the window of win_length samples
 * is zero-padded to n_fft and centred as torch.stft does.  A general plan serves aware_stft, aware_istft, aware_stft_bwd
 * and aware_istft_bwd on batches made by aware_batch_create_for_plan, with any band arguments.  Created with the flag
 * AWARE_PLAN_GENERAL (below) and a band inside bins 0..n_fft/2 it also serves the loop on the GENERAL ROUTE (csrc/loop_any.hip): aware_detector_create[_ex],
 * aware_detect, aware_embed_create / _begin / _iterate / _gradient / _profile / _finish / _buffer and
 * aware_embed_set_optimizer, with a batch made for that plan and a detector created for it (anything else: AWARE_E_BADARG;
 * a band outside the spectrum: AWARE_E_UNSUPPORTED from aware_detector_create).  A general plan created without the flag
 * is a plan for the transforms alone: aware_detector_create, aware_detect and aware_embed_create return
 * AWARE_E_UNSUPPORTED for it before they read another argument, as they always did.  The mel basis handed to
 * aware_detector_create is then [n_mels][n_fft/2 + 1].  Not on a general plan: aware_stft_band, the loop attacks and
 * mixtures and the loss AWARE_LOSS_PUSH_L1 (AWARE_E_UNSUPPORTED), aware_detector_forward / _backward and the training entry
 * points (AWARE_E_BADARG for a general batch).  aware_embed_create also refuses (AWARE_E_BADARG) a batch with a clip that
 * fails aware_nola_check or is shorter than one hop.
 * aware_plan_create_ex: flags AWARE_PLAN_GENERAL builds a general plan even for the card geometry (tests hold the two
 * paths against each other) and opens the loop on the plan, whatever its geometry.  aware_plan_create(...) == aware_plan_create_ex(..., 0). */
#define AWARE_PLAN_GENERAL 1
int aware_plan_create_ex(aware_plan** out, int n_fft, int hop, int win_length, int window, int band_lo_bin,
                         int band_hi_bin, int flags);
/* complex values per frame row of the plan's spectra: AWARE_FULL_STRIDE (520) for the card plan, n_fft/2 + 1 rounded up
 * to a multiple of 8 for a general plan (bins 0..n_fft/2 valid, the rest written as zero) */
int aware_plan_spectrum_stride(const aware_plan* plan);
/* 1 for a general plan, 0 for the card plan */
int aware_plan_is_general(const aware_plan* plan);
/* floats per row of the plan's band-limited arrays: AWARE_SPEC_STRIDE or AWARE_SPEC_STRIDE_WIDE for a card plan; for a
 * general plan the band's bins rounded up to a multiple of 64 (2112 for all 2049 bins of n_fft 4096; AWARE_SPEC_STRIDE when
 * its band lies outside the spectrum).  The *_workspace_bytes functions count rows of this stride. */
int aware_plan_band_stride(const aware_plan* plan);
/* torch.istft's NOLA condition (host only, no device): AWARE_OK when the overlap-add envelope of this geometry stays
 * >= 1e-11 over the trimmed output of a clip of n_samples samples (T = 1 + n_samples/hop frames), AWARE_E_BADARG when
 * torch.istft would raise for it (aware_istft / aware_istft_bwd refuse such a batch with AWARE_E_BADARG) */
int aware_nola_check(int n_fft, int hop, int win_length, int window, int n_samples);

/* ---- batch geometry ----------------------------------------------------------------------
 * n_samples[B] (host): clip lengths.  in_offsets[B] (host, may be NULL = densely packed):
 * float offset of clip b inside the caller's ragged audio array. */
int aware_batch_create(aware_batch** out, int B, const int* n_samples, const int* in_offsets);
void aware_batch_destroy(aware_batch* batch);
int aware_batch_total_frames(const aware_batch* batch);   /* sum T_b          */
int aware_batch_total_pooled(const aware_batch* batch);   /* sum T_b/2        */
int aware_batch_total_out(const aware_batch* batch);      /* sum 256*(T_b-1)  */
int aware_batch_out_offset(const aware_batch* batch, int b); /* float offset of clip b's output */
int aware_batch_out_length(const aware_batch* batch, int b);
int aware_batch_frames(const aware_batch* batch, int b);
/* read-only: the run lengths aware_batch_create chose for this batch -- hop blocks per workgroup segment of the synthesis
 * side (and of every embed-loop attack kernel), 16 / 12 / 8 / 6 / 4, and frames per analysis run, 4..12 (a general batch,
 * which has no streaming kernels, reports 16 and 0).  For tests and logs; nothing can set them. */
int aware_batch_synth_run(const aware_batch* batch);
int aware_batch_analysis_run(const aware_batch* batch);
/* a batch for a plan: frames T_b = 1 + n_b/hop by the plan's hop, istft outputs hop*(T_b - 1) samples, clips need more than
 * n_fft/2 samples (AWARE_E_BADARG otherwise).  For the card plan the same as aware_batch_create.  A general batch also holds
 * the overlap-add frame buffer of the synthesis direction ([total frames][n_fft] floats, allocated here), so one general batch
 * must not be used on two streams at the same time.  It has T_b/2 pooled frames per clip like a card batch
 * (aware_batch_total_pooled), and aware_detect_workspace_bytes / aware_embed_workspace_bytes are exact for it: one byte
 * less is AWARE_E_WORKSPACE. */
int aware_batch_create_for_plan(aware_batch** out, const aware_plan* plan, int B, const int* n_samples,
                                const int* in_offsets);

/* ---- DSP plug-ins ---------------------------------------------------------------------------
 * aware_stft: WaveformNormalizer (optional) + STFT.__call__  (utils/audio/waveform.py:18-19,
 * utils/audio/stft.py:27-28).  audio: dev ragged f32.  spec: dev complex64
 * [total frames][AWARE_FULL_STRIDE] (bins 0..512 valid).  normalize: 0 none, 1 x/max(|x|+1e-8).
 * scratch: dev, >= aware_batch_scratch_bytes(). */
size_t aware_batch_scratch_bytes(const aware_batch* batch);
int aware_stft(const aware_plan* plan, const aware_batch* batch, const float* audio, int normalize,
               void* spec, void* scratch, void* stream);
/* aware_istft: ISTFT.__call__ (utils/audio/stft.py:47-48; no length argument, output
 * 256*(T-1) samples per clip at aware_batch_out_offset).  normalize as above, applied to the output. */
int aware_istft(const aware_plan* plan, const aware_batch* batch, const void* spec, int normalize,
                float* out, void* scratch, void* stream);
/* aware_stft_band: normalise + STFT + STFTDecomposer restricted to the embedding band:
 * mag [total frames][stride] and unit phasor (cos, sin of the phase) [total frames][stride] complex64, stride =
 * aware_plan_band_stride(plan).  DC and Nyquist, when in the band, have phasor (+-1, 0) as torch.angle gives 0 / pi. */
int aware_stft_band(const aware_plan* plan, const aware_batch* batch, const float* audio, int normalize,
                    float* mag, void* phasor, void* scratch, void* stream);

/* Backward passes of the two transforms for the differentiable plug-in seam (BaseAudioProcessor.__call__,
 * interfaces/audio.py:6-9; what torch autograd derives for torch.stft / torch.istft inside
 * embedding/multibit_embedder.py:49-67).  Gradients of a real loss; complex gradients in torch's convention
 * (dL/dRe + i dL/dIm).
 * aware_stft_bwd: grad_spec dev complex64 [total frames][AWARE_FULL_STRIDE] -> grad_audio dev f32, laid out like the audio
 *   aware_stft takes (clip b: n_b samples at in_offsets[b]): any clip length n > 512, ragged batches (the reflect pads fold
 *   about sample 0 and sample n - 1).
 * aware_istft_bwd: grad_audio dev f32 [total out] -> grad_spec dev complex64 [total frames][AWARE_FULL_STRIDE].
 * General plans: the four transforms take spectra of aware_plan_spectrum_stride(plan) complex values per row, clips of any
 * length n > n_fft/2, hop*(T-1) output samples per clip; aware_istft / aware_istft_bwd return AWARE_E_BADARG for a batch
 * that violates the NOLA condition (aware_nola_check) and every entry point returns it for a batch not made for the plan. */
int aware_stft_bwd(const aware_plan* plan, const aware_batch* batch, const void* grad_spec, float* grad_audio,
                   void* stream);
int aware_istft_bwd(const aware_plan* plan, const aware_batch* batch, const float* grad_audio, void* grad_spec,
                    void* stream);

/* The element-wise plug-ins and the optimiser step of the reference's loop, with their backward passes, for the same
 * seam (n = number of complex / real elements; all pointers dev):
 *   aware_polar_decompose      STFTDecomposer: (|S|, angle S)  utils/audio/stft.py:54-55  (phase may be NULL)
 *   aware_polar_assemble       STFTAssembler: mag * exp(i phase)  utils/audio/stft.py:61-62
 *   aware_waveform_normalize_bwd  backward of x / max(|x| + 1e-8), utils/audio/waveform.py:18-19 (through the max)
 *   aware_nadam_clamp_step     torch.optim.NAdam single-tensor step + torch.clamp(coeffs, lo, hi)
 *                              (embedding/multibit_embedder.py:112-117); coef3 = the three per-step scalars written by
 *                              aware_nadam_coefficients (host; mu_product_io carries torch's mu_product between steps,
 *                              start it at 1.0f; step counts from 1).  Same arithmetic as the fused loop. */
int aware_polar_decompose(const void* spec, float* mag, float* phase, size_t n, void* stream);
int aware_polar_decompose_bwd(const void* spec, const float* grad_mag, const float* grad_phase, void* grad_spec, size_t n,
                              void* stream);
int aware_polar_assemble(const float* mag, const float* phase, void* spec, size_t n, void* stream);
int aware_polar_assemble_bwd(const float* mag, const float* phase, const void* grad_spec, float* grad_mag,
                             float* grad_phase, size_t n, void* stream);
int aware_waveform_normalize_bwd(const float* in, const float* grad_out, float* grad_in, const int* off, const int* len,
                                 int B, void* stream);
int aware_nadam_coefficients(int step, float lr, float beta1, float beta2, float momentum_decay, float* mu_product_io,
                             float* coef3);
int aware_nadam_clamp_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const float* lo,
                           const float* hi, size_t n, const float* coef3, float beta1, float beta2, float eps, void* stream);

/* ---- detector --------------------------------------------------------------------------------
 * AWAREDetectorNet (detection/multibit_detector_net.py:17-80).  All arrays are host fp32:
 * mel_basis [n_mels][n_fft/2+1] (detection/modules/mel.py:105-149), conv weights
 * [channels[i+1]][channels[i]] and biases [channels[i+1]] for i < n_layers
 * (channels = {128, 512, 1024, 1024, 40}).  The library uploads and pre-transposes them.
 * channels[0] = n_mels, 1..512; channels[1 .. n_layers-1] (hidden widths) 1..4096; n_layers 1..33 (num_blocks 0..32);
 * channels[n_layers] = 2 * payload bits, any even value from 2 to 1024 (payloads of 1..512 bits), else AWARE_E_UNSUPPORTED.
 * Storage rule: n_mels and every hidden width are stored as given when a multiple of 4, else rounded up to a multiple of 4
 * (up to 64) or of 128 (above 64); the last block is rounded up to a multiple of 4 up to 64 and of 128 above.  Padding
 * channels have zero weights, biases and mel rows (BatchNorm: scale 0, shift 0), are never read out and get a zero
 * gradient.  Every array the caller passes or receives keeps the caller's shapes.  The training extension
 * (aware_detector_update*, aware_detector_*_gradients) serves n_mels = 128, hidden widths that are multiples of 4 and at
 * most 7 layers only (AWARE_E_UNSUPPORTED otherwise). */
int aware_detector_create(aware_detector** out, const aware_plan* plan, const float* mel_basis, int n_mels,
                          int n_layers, const int* channels, const float* const* weights,
                          const float* const* biases);
void aware_detector_destroy(aware_detector* det);

/* Architecture variants of the network (detection_net_cfg of the model card; modules/conv1d.py:8-36 and
 * multibit_detector_net.py:82-96).  activation: the activation of every conv block; norm: its norm -- INSTANCE =
 * InstanceNorm1d (no affine, biased variance, eps 1e-5, per clip over time), BATCH = BatchNorm1d in eval mode, given as the
 * per-channel affine map u = z * norm_scale[l][c] + norm_shift[l][c] (scale = gamma / sqrt(running_var + eps), shift =
 * beta - running_mean * scale; host arrays of channels[l+1] floats for every l < n_layers, BATCH only, may be NULL
 * otherwise), NONE = identity (the conv bias reaches the activation); final_activation: the activation of the bitwise
 * read-out head, applied to even - odd.  LEAKY_RELU has slope 0.2, GELU is the exact erf form, SWISH is SiLU; at the kinks
 * the derivatives are torch's (ReLU'(0) = 0, LeakyReLU'(0) = 0.2).
 * aware_detector_create_ex(..., arch) with {LEAKY_RELU, INSTANCE, TANH} is aware_detector_create: the model card's network,
 * served by the fused conv-block, read-out and tail kernels.  Every other architecture runs the staged route (plain GEMM +
 * bias, a norm / activation kernel, the read-out kernel; a batch-sized stash of pre-activations per block in the workspace,
 * counted by the *_workspace_bytes functions) through aware_detect, aware_detector_forward / _backward and the aware_embed_*
 * loop, with no other entry point.  The training extension (aware_detector_train_gradients, _weight_gradients, _update,
 * _update_device) returns AWARE_E_UNSUPPORTED for it.  Enum values out of range: AWARE_E_BADARG; a general plan:
 * AWARE_E_UNSUPPORTED. */
#define AWARE_ACT_RELU 0
#define AWARE_ACT_LEAKY_RELU 1
#define AWARE_ACT_GELU 2
#define AWARE_ACT_SWISH 3
#define AWARE_NORM_INSTANCE 0
#define AWARE_NORM_BATCH 1
#define AWARE_NORM_NONE 2
#define AWARE_FINAL_RELU 0
#define AWARE_FINAL_LEAKY_RELU 1
#define AWARE_FINAL_GELU 2
#define AWARE_FINAL_SWISH 3
#define AWARE_FINAL_TANH 4
#define AWARE_FINAL_SIGMOID 5
typedef struct aware_detector_arch {
    int activation;                      /* AWARE_ACT_*   */
    int norm;                            /* AWARE_NORM_*  */
    int final_activation;                /* AWARE_FINAL_* */
    const float* const* norm_scale;      /* AWARE_NORM_BATCH: [n_layers] host arrays [channels[l+1]] */
    const float* const* norm_shift;
} aware_detector_arch;
int aware_detector_create_ex(aware_detector** out, const aware_plan* plan, const float* mel_basis, int n_mels,
                             int n_layers, const int* channels, const float* const* weights,
                             const float* const* biases, const aware_detector_arch* arch);
/* 1 when the detector has the model card's architecture (fused kernels), 0 for a variant (staged route) */
int aware_detector_is_card(const aware_detector* det);

/* Temporal convolutions (kernel_size, stride and padding of detection_net_cfg; modules/conv1d.py; added without a version
 * step, so a caller detects them by symbol): every one of the n_layers blocks is Conv1d(channels[l], channels[l+1],
 * kernel_size, stride, padding) -> norm -> activation along the pooled frames.  A clip of L_0 = floor(frames / 2) pooled rows
 * leaves block l with L_{l+1} = floor((L_l + 2 padding - kernel_size) / stride) + 1 rows; InstanceNorm runs over the block's
 * rows and the read-out mean over the last block's.  weights[l]: host [channels[l+1]][channels[l]][kernel_size] (torch's
 * Conv1d layout).  Served: kernel_size 1..7, stride 1..4, 2 padding <= kernel_size - 1 (no block is then longer than its
 * input); outside that AWARE_E_UNSUPPORTED, non-positive sizes AWARE_E_BADARG.  1 / 1 / 0 is aware_detector_create_ex.
 * Every other detector made here runs the staged route in every block whatever its arch is: unfold, plain GEMM with K =
 * kernel_size * channels[l], the norm / activation kernel, the read-out kernel; aware_detector_is_card is 0, the training
 * extension returns AWARE_E_UNSUPPORTED, and the *_workspace_bytes functions count one scratch of total pooled rows x
 * kernel_size x the widest block input.  A batch with a clip that some block leaves without a row (torch raises there) is
 * refused with AWARE_E_BADARG by aware_detect, aware_detector_forward / _backward and aware_embed_create. */
int aware_detector_create_conv(aware_detector** out, const aware_plan* plan, const float* mel_basis, int n_mels,
                               int n_layers, const int* channels, const float* const* weights,
                               const float* const* biases, const aware_detector_arch* arch, int kernel_size, int stride,
                               int padding);
/* the kernel_size, stride and padding of a detector (1 / 1 / 0 for one of 1x1 convolutions); any pointer may be NULL */
int aware_detector_conv(const aware_detector* det, int* kernel_size, int* stride, int* padding);
/* rows left of `rows` pooled rows behind `blocks` blocks (0 once a block has no output row) */
int aware_conv_rows(int rows, int blocks, int kernel_size, int stride, int padding);
/* The two data-movement kernels of such a block on their own.  x / dx: dev f32 [total pooled rows][channels], u / du: dev f32
 * [total pooled rows][kernel_size * channels], channels % 4 == 0; clip b's rows start at its 32-aligned pooled offset.
 * unfold (block's input -> GEMM operand): u[r0 + t][j * channels + c] = x[r0 + t * stride - padding + j][c] inside the
 * clip's L_block rows, else 0, for t < L_{block+1}; the rows up to the clip's 32-row boundary are written as zeros.  fold:
 * its adjoint, dx[r0 + q][c] = the sum over j ascending of du[r0 + t][j * channels + c] with t * stride - padding + j = q. */
int aware_conv_unfold(const aware_batch* batch, const float* x, float* u, int channels, int block, int kernel_size,
                      int stride, int padding, void* stream);
int aware_conv_fold(const aware_batch* batch, const float* du, float* dx, int channels, int block, int kernel_size,
                    int stride, int padding, void* stream);

/* Initial pools (initial_pool_size and initial_pool_stride of detection_net_cfg; multibit_detector_net.py:53, 131; added
 * without a version step, so a caller detects them by symbol): the AvgPool1d(pool_size, pool_stride) between the mel stage
 * and block 0.  A clip of T frames enters block 0 with L_0 = aware_pool_rows(T, pool_size, pool_stride) =
 * floor((T - pool_size) / pool_stride) + 1 rows, 0 for T < pool_size; the frames from (L_0 - 1) pool_stride + pool_size on are
 * dropped by the pool and still count in the mel stage's InstanceNorm and GlobalStandardize.  Served: pool_size 2..8 and
 * pool_stride 2..8 in any combination (windows overlap where pool_size > pool_stride and leave gaps where it is smaller);
 * outside that AWARE_E_UNSUPPORTED, non-positive values AWARE_E_BADARG.  From 2 on L_0 <= floor(T / 2), so batches and
 * workspaces are what they are for every other detector; a size or stride of 1 is not served.  The other arguments are those
 * of aware_detector_create_conv, and 2 / 2 is that function.  Every other detector made here runs the staged route whatever
 * its arch is: the mel stage's normalise-and-pool kernels for any pool, then per block the plain GEMM (behind the unfold for
 * temporal convolutions) and the norm / activation kernel over the block's own rows, then the read-out kernel;
 * aware_detector_is_card is 0 and the training extension returns AWARE_E_UNSUPPORTED.  A batch with a clip that the pool or
 * a later block leaves without a row is refused with AWARE_E_BADARG by aware_detect, aware_detector_forward / _backward and
 * aware_embed_create. */
int aware_detector_create_pool(aware_detector** out, const aware_plan* plan, const float* mel_basis, int n_mels,
                               int n_layers, const int* channels, const float* const* weights,
                               const float* const* biases, const aware_detector_arch* arch, int kernel_size, int stride,
                               int padding, int pool_size, int pool_stride);
/* the initial pool of a detector (2 / 2 for every detector not made by aware_detector_create_pool); either pointer may be NULL */
int aware_detector_pool(const aware_detector* det, int* pool_size, int* pool_stride);
/* rows a clip of `frames` frames has behind the pool (0 for frames < pool_size); aware_pool_rows(T, 2, 2) == T / 2 */
int aware_pool_rows(int frames, int pool_size, int pool_stride);

/* AWAREDetector.detect (detection/multibit_detector.py:28-42), batched: normalise, STFT, |.|,
 * zero the out-of-band bins, network forward.  values: dev f32 [B][n_bits].
 * workspace: dev, >= aware_detect_workspace_bytes(). */
size_t aware_detect_workspace_bytes(const aware_batch* batch, const aware_detector* det);
int aware_detect(const aware_plan* plan, const aware_detector* det, const aware_batch* batch,
                 const float* audio, float* values, void* workspace, size_t workspace_bytes, void* stream);
/* network forward only (AWAREDetectorNet.forward, :109-140) on a band magnitude array */
int aware_detector_forward(const aware_detector* det, const aware_batch* batch, const float* mag,
                           float* values, void* workspace, size_t workspace_bytes, void* stream);

/* forward + backward of the network for the differentiable seam (BaseDetectorNet.forward, interfaces/detection.py:10-14,
 * under autograd): values [B][n_bits] (may be NULL) and grad_mag [total frames][band stride] = J^T grad_values; data gradients
 * only (the reference freezes the weights, multibit_embedder.py:76-77). */
size_t aware_detector_backward_workspace_bytes(const aware_batch* batch, const aware_detector* det);
int aware_detector_backward(const aware_detector* det, const aware_batch* batch, const float* mag,
                            const float* grad_values, float* values, float* grad_mag, void* workspace,
                            size_t workspace_bytes, void* stream);

/* EXTENSION -- detector training step (BASELINE.json north_star: "RCCL all-reduce over xGMI on the embedder/detector
 * gradients"; the reference freezes the detector, multibit_embedder.py:76-77, and trains nothing: parity unpinned, specified
 * by torch autograd on the oracle's Detector).  aware_detector_weight_gradients = aware_detector_backward plus
 * dL/dW_l [Cout][Cin] and dL/db_l [Cout] of every conv block (grad_weights / grad_biases: host arrays of n_layers device
 * pointers, entries may be NULL, each on its own); the caller all-reduces them over its ranks, applies its optimiser and
 * writes the new parameters back with aware_detector_update (host arrays as for aware_detector_create, same shapes,
 * synchronous).
 * The gradient entry points serve detectors of a narrow-layout band only: AWARE_E_UNSUPPORTED for the wide layout. */
size_t aware_detector_train_workspace_bytes(const aware_batch* batch, const aware_detector* det);
int aware_detector_weight_gradients(const aware_detector* det, const aware_batch* batch, const float* mag,
                                    const float* grad_values, float* values, float* grad_mag,
                                    float* const* grad_weights, float* const* grad_biases, void* workspace,
                                    size_t workspace_bytes, void* stream);
int aware_detector_update(aware_detector* det, const float* mel_basis, const float* const* weights,
                          const float* const* biases);
/* the step without host round trips: aware_detector_train_gradients evaluates the loss inside (ONE forward + backward; target
 * [B][n_bits] bipolar, loss_kind 0..5 as the embed loop, loss_out dev [B]; the gradients are those of the SUM of the per-clip
 * losses; grad_mag may be NULL), aware_detector_update_device rebuilds every device image of the parameters from DEVICE arrays
 * (asynchronous on `stream`; dev_weights / dev_biases: host arrays of device pointers, biases may be NULL). */
int aware_detector_train_gradients(const aware_detector* det, const aware_batch* batch, const float* mag, const float* target,
                                   int loss_kind, float* loss_out, float* values, float* grad_mag,
                                   float* const* grad_weights, float* const* grad_biases, void* workspace,
                                   size_t workspace_bytes, void* stream);
int aware_detector_update_device(aware_detector* det, const float* const* dev_weights, const float* const* dev_biases,
                                 void* stream);

/* ---- embedder -----------------------------------------------------------------------------------
 * AWAREEmbedder.embed / _optimize (embedding/multibit_embedder.py:70-197), batched and ragged:
 * every clip is its own optimisation problem.  loss: AWARE_LOSS_* above -- 0 push_extremes, 1 mse, 2 hinge, 3 sign,
 * 4 push_sigmoid, 5 ber (no gradient) (embedding/losses.py:95-103), 6 push_extremes + L1 (EXTENSION, streaming DSP path
 * only), 8 bce (a detector that ends in AWARE_FINAL_SIGMOID only, on every route such a detector takes; the training entry
 * points refuse it).  optimizer: NAdam (embedding/optimizers.py:5; torch.optim.NAdam
 * single-tensor semantics) with lr, beta1, beta2, eps, momentum_decay; the reference's
 * ReduceLROnPlateau(patience 500) never fires within 400 iterations and is not modelled. */
typedef struct aware_embed_config {
    int num_iterations;      /* cards/config.yaml:16  (400) */
    float tolerance_db;      /* cards/config.yaml:13  (6.0) */
    int loss;                /* 0 = push_extremes */
    float lr, beta1, beta2, eps, momentum_decay;   /* 0.1, 0.9, 0.999, 1e-8, 4e-3 */
    int use_graph;           /* 1: capture one iteration into a hipGraph and replay it */
    /* kernel choices of this session (zero = default).
     * conv_pipe 0: the conv blocks and their data-gradient GEMMs of a uniform batch that fills the chip run on the f16 matrix
     *   pipe: every f32 operand scaled by a power of two (per output channel / per clip) and written as two binary16 terms
     *   (representation error <= one f32 ulp, rms 2^-24.5; l_a l_b dropped), three partial products per multiply-add, f32 accumulation
     *   (csrc/gemm_h2.hip); every other GEMM as conv_pipe 2.
     * conv_pipe 2: the detector's GEMMs on the bf16 matrix pipe with every f32 operand split exactly into three
     *   bf16 terms, six partial products per multiply-add, f32 accumulation (csrc/gemm_x3.hip) wherever K % 64 == 0 and
     *   N % 128 == 0, f32 MFMA otherwise.
     * conv_pipe 1: f32-input MFMA everywhere (the pipe the 16-bit kernels are tested against).
     * All three agree with fp64 to f32 rounding level (tests/test_gpu_kernels.py::test_gemm_clip_x3).
     * readout 0: fused read-out kernel on uniform batches; 1: split-K GEMM + tail kernel + data-gradient GEMM (the
     *   path ragged batches take). */
    int conv_pipe;
    int readout;
    /* dsp_path 0: streaming wave kernels for the framed STFT / iSTFT and their adjoints (csrc/dsp_stream.hip: one wave
     *   streams a run of frames, overlap-add and frame overlap in registers, no barrier) wherever the band lies inside
     *   bins 1..256 or has the wide layout; 1: workgroup-staged kernels (csrc/dsp_kernels.hip: any band; the form the streaming kernels are
     *   tested against). */
    int dsp_path;
    /* loss AWARE_LOSS_PUSH_L1 only (EXTENSION, BASELINE config 3 "BER + L1"; the reference's imperceptibility device is
     * the box constraint :157-160, which stays in force): weight of mean|c - c0| over a clip's 225*T coefficients */
    float l1_weight;
    /* mel 0: the mel projection's backward runs as two taps per bin inside the streaming synthesis adjoint (a triangular filter
     *   bank -- detection/modules/mel.py:105-149 -- has at most two adjacent non-zero weights per FFT bin; dL/d|S| is never
     *   stored) whenever dsp_path is 0, the band has the narrow layout and the detector's basis has that form; 1: the dense
     *   [NF][128] x [128][stride] GEMM (the only form of a band with the wide layout)
     *   (what the fused form is tested against). */
    int mel;
    /* conv_tile (conv_pipe 0, uniform batches): the form of the f16 two-term conv kernel.  0: chosen per launch when the
     *   session plans its kernels -- the wide form (4 waves x 64 columns per workgroup, 256-column slabs, csrc/gemm_h2.hip) where
     *   it can run (at most 96 pooled rows per clip, N % 256 == 0) and its grid still fills the chip, else the 128-column form;
     *   1: the 128-column form everywhere; 2: the wide form wherever it can run (AWARE_E_UNSUPPORTED from aware_embed_create
     *   when no conv launch of the session can take it).  The forms give the same bits.  (Added at the end of the struct
     *   without a version step: a caller finds it by the symbol aware_embed_conv_tile.) */
    int conv_tile;
} aware_embed_config;

/* ---- optimiser / scheduler registries (the reference's third seam: embedding/optimizers.py:3-20, schedulers.py:3-16) ------
 * The model card's NAdam + never-firing ReduceLROnPlateau runs fused in the adjoint kernel's epilogue (aware_embed_config).
 * Any other registered optimiser / schedule: the HOST computes the per-step scalars of torch's single-tensor update under
 * the chosen learning-rate schedule, the device applies them in one element-wise launch per iteration (+ clamp, + best
 * snapshot).  kind: AWARE_OPT_*.  table: HOST [num_iterations][5] doubles per step t = 1..: (ux, uy, z, lr_t, h0_t) with
 * c.x = lr*ux, c.y = lr*uy (sgd: uy = 1 on the first step), c.z = z, h0_t >= 0 overrides hyp[0] (1 - beta1, or the momentum
 * of sgd / rmsprop: CyclicLR cycles it); hyp: see csrc/dsp_args.hpp::opt_clamp_update (rmsprop: hyp[0] = momentum, 0 = none;
 * with it state1 is torch's momentum buffer).  plateau != 0: torch's ReduceLROnPlateau (mode min, rel
 * threshold, cooldown 0) with one state PER CLIP, stepped with the clip's loss after each optimiser step; lr0 = initial rate.
 * Call after aware_embed_create and before the first aware_embed_iterate. */
#define AWARE_OPT_NADAM 0
#define AWARE_OPT_ADAM 1
#define AWARE_OPT_ADAMW 2
#define AWARE_OPT_SGD 3
#define AWARE_OPT_RMSPROP 4
#define AWARE_OPT_ADAGRAD 5
#define AWARE_OPT_ADAMAX 6
#define AWARE_OPT_ADADELTA 7
typedef struct aware_optimizer_config {
    int kind;
    float hyp[8];
    double weight_decay;      /* adamw only (decoupled); the L2 form of the others travels in hyp[4] */
    const double* table;
    int plateau, patience;
    double factor, threshold, min_lr, eps, lr0;
} aware_optimizer_config;
int aware_embed_set_optimizer(aware_embed* e, const aware_optimizer_config* cfg, void* stream);
/* the same update on the caller's flat tensors, for the plug-in loop (generalises aware_nadam_clamp_step): coef4 = the
 * step's (c.x, c.y, c.z, c.w) as float, hyp8 as above; state1 = exp_avg / momentum buffer / acc_delta, state2 = exp_avg_sq /
 * square_avg / state_sum / exp_inf */
int aware_opt_clamp_step(int kind, float* param, const float* grad, float* state1, float* state2, const float* lo,
                         const float* hi, size_t n, const float* coef4, const float* hyp8, void* stream);

size_t aware_embed_workspace_bytes(const aware_batch* batch, const aware_detector* det);
int aware_embed_create(aware_embed** out, const aware_plan* plan, const aware_detector* det,
                       const aware_batch* batch, const aware_embed_config* cfg, void* workspace,
                       size_t workspace_bytes, void* stream);
void aware_embed_destroy(aware_embed* e);
/* read-only, for tests and logs: the form the session's plan gives the conv launch of block `layer` (backward 0: the block's
 * forward, 1: its data-gradient GEMM): 2 = the wide form of the f16 two-term kernel, 1 = its 128-column form, 0 = the launch
 * runs on another kernel (or does not exist); AWARE_E_BADARG for a layer outside 0 .. n_layers - 1. */
int aware_embed_conv_tile(const aware_embed* e, int backward, int layer);
/* analysis, bounds, optimiser reset.  audio: dev ragged f32 (un-normalised); target: dev f32
 * [B][n_bits] bipolar (+-1), PatternEncoder output (utils/watermark/encoder.py:35-45). */
int aware_embed_begin(aware_embed* e, const float* audio, const float* target, void* stream);
/* n_iters loop bodies (:95-122): synth -> normalise -> analysis -> detector fwd -> loss ->
 * backward -> NAdam -> clamp -> best snapshot.  No host synchronisation.  AWARE_E_BADARG when more than
 * cfg.num_iterations steps would have run since aware_embed_begin (the reference's loop runs exactly that many). */
int aware_embed_iterate(aware_embed* e, int n_iters, void* stream);
/* forward + backward without the optimiser step and without best-loss bookkeeping; grad: dev f32
 * [total frames][band stride] = dL/dcoef; loss[] and pred[] (aware_embed_buffer 0, 2) are refreshed */
int aware_embed_gradient(aware_embed* e, float* grad, void* stream);
/* Timing aid for the roofline report: runs n_iters loop bodies eagerly with a HIP event recorded on
 * `stream` after every kernel launch; writes the elapsed milliseconds between consecutive events and
 * a kernel kind per launch (0 synth, 1 analysis, 2 generic gemm, 3 mel-norm, 4 in+lrelu, 5 read-out/tail,
 * 6 synth adjoint, 7 analysis adjoint + NAdam, 8 misc, 9 clip-aligned gemm with fused forward
 * epilogue, 10 the same with fused backward epilogue).  Synchronises the stream.  Returns the number of
 * entries written or a negative error.  (These iterations DO step the optimiser and count against
 * cfg.num_iterations like aware_embed_iterate.) */
int aware_embed_profile(aware_embed* e, int n_iters, int max_entries, float* ms_out, int* kind_out, void* stream);
/* final synthesis from the best coefficients (:173-194) and the service-level rescale
 * (service/embed.py:69,73): out[b] = rescale[b] * normalise(istft(...)).  rescale: dev f32 [B] or NULL. */
int aware_embed_finish(aware_embed* e, const float* rescale, float* out, void* stream);
/* device pointers to internal state for inspection: 0 loss[B], 1 best_loss[B], 2 pred[B][n_bits],
 * 3 coef [frames][band stride], 4 best coef, 5 lo, 6 hi, 7 phasor (complex64), 8 step counter (int32), 9 un-normalised synthesis,
 * 10 band magnitudes of the last analysis, 11 per-clip learning rates (f64 [B]; NULL unless aware_embed_set_optimizer ran),
 * 12 the attacked signal z of the last forward pass (layout of 9; NULL unless aware_embed_set_loop_attacks or, on a
 *    general plan, aware_embed_set_general_chain set a chain)
 * 13 the impulse responses of the last forward pass (NULL unless the chain has a reverberation; see below)
 * 14 the choices of the last forward pass, int32 [B] (NULL unless aware_embed_set_loop_mixture set a mixture; see below) */
void* aware_embed_buffer(aware_embed* e, int which);

/* ---- attacks (scripts/attacks.py) ------------------------------------------------------------------
 * All operate on ragged batches given by dev int32 arrays off[B], len[B]. */
/* PCMBitDepthConversion.apply :44-70. bits in {8,12,16,24}.  scratch >= B*(ceil(max_len/4096)*8 + 4) bytes */
int aware_pcm_quantize(const float* in, float* out, const int* off, const int* len, int B, int max_len,
                       int bits, void* scratch, void* stream);
/* WaveformNormalizer.__call__ (src/AWARE/utils/audio/waveform.py:18-19) as a stand-alone op:
 * out = in / max(|in| + 1e-8) per clip.  scratch as for aware_pcm_quantize (+ 4*B bytes). */
int aware_waveform_normalize(const float* in, float* out, const int* off, const int* len, int B, int max_len,
                             void* scratch, void* stream);
/* scipy.signal.resample_poly's polyphase core (Resample.apply :290-293, scripts/test.py:60-63):
 * out[j] = sum_i in[i] * h[j*down - i*up + half_len], fp32.  h: dev f32 [nh] (already scaled by up), nh >= 1 and
 * half_len >= 0.  Any nh is served: with nh < up some output phases meet no tap, and those outputs are 0. */
int aware_upfirdn(const float* in, const int* in_off, const int* in_len, float* out, const int* out_off,
                  const int* out_len, int B, int max_out, const float* h, int nh, int up, int down,
                  int half_len, void* stream);
/* Resample.apply's branch for sr // target_sr = factor > 1 (scripts/attacks.py:275-288): keep every factor-th sample
 * and linearly interpolate back to the original length with np.interp's float64 arithmetic.  out: dev f64 at the
 * same offsets as `in`. */
int aware_decimate_interp(const float* in, const int* off, const int* len, int B, int max_len, int factor,
                          double* out, void* stream);
/* scipy.signal.lfilter (LowPassFilter / HighPassFilter :400-455) and filtfilt (RandomBandstop
 * :324-356) in f64.  b, a: dev f64 [B][ncoef] (a[0] == 1); zi: dev f64 [B][ncoef-1] (filtfilt only).
 * out is f64 when out_f64 != 0 (the reference returns float64 from lfilter), else f32.
 * scratch (filtfilt): dev f64 [B][max_len + 6*ncoef].  2 <= ncoef <= 12.  A filtfilt clip must be longer than the
 * padding of 3*ncoef samples (scipy raises for such a clip; the host binding does the same, the kernel only stays inside
 * its buffers).  PRECONDITION: every len[b] >= 1.  The lengths live on the device, so this call cannot check them: the
 * host binding refuses a batch with an empty clip, and a direct caller must do the same (the kernel leaves an empty
 * clip's workgroup at once and writes nothing for it).  One workgroup per clip, parallel in time (128 chunks chained
 * with a double-double state transition): results agree with scipy's sequential recurrence to the rounding of that recurrence itself. */
int aware_iir(const float* in, const int* off, const int* len, int B, int max_len, void* out, int out_f64,
              const double* b, const double* a, const double* zi, int ncoef, int filtfilt,
              void* scratch, void* stream);
/* DeleteSamples :162-178 / Cropout :192-205 (zero_fill = 0) and SampleSupression :370-385
 * (zero_fill = 1): cut_start[B], cut_len[B] dev int32 chosen by the host RNG. */
int aware_segment_cut(const float* in, const int* in_off, float* out, const int* out_off, const int* out_len,
                      const int* cut_start, const int* cut_len, int zero_fill, int B, int max_len, void* stream);
/* EXTENSION (not in the reference): additive Gaussian noise at snr_db, Philox-4x32-10 keyed by
 * seeds[b].  scratch >= B*8 bytes. */
int aware_gaussian_noise(const float* in, float* out, const int* off, const int* len, int B, int max_len,
                         const uint32_t* seeds, float snr_db, void* scratch, void* stream);

/* EXTENSION (not in the reference): MP3-like quantisation surrogate on a full one-sided spectrum
 * [n_frames][AWARE_FULL_STRIDE] complex64, in place: per frame the magnitudes are quantised on a
 * step_db grid relative to the frame maximum and zeroed below floor_db; the phase is kept.
 * Used as  aware_stft -> aware_spectral_quantize -> aware_istft. */
int aware_spectral_quantize(void* spec, int n_frames, float step_db, float floor_db, void* stream);
/* Its backward, which makes the surrogate a DIFFERENTIABLE op (north_star: "differentiable MP3-like quantisation
 * surrogates"; the reference's MP3Compression, scripts/attacks.py:73-148, shells out to ffmpeg and has no gradient):
 * straight-through on the magnitude (dQ/d|X| := 1 on kept bins, 0 on bins dropped below the floor, frame maximum constant),
 * exact through the phase.  spec_in: the spectrum BEFORE quantisation; grad_out = dL/dRe Y + i dL/dIm Y; grad_in likewise for
 * X; all dev complex64 [n_frames][AWARE_FULL_STRIDE].  Specified by oracle/aware_oracle.py::mp3_surrogate_spectrum under torch
 * autograd (parity unpinned: extension). */
int aware_spectral_quantize_bwd(const void* spec_in, const void* grad_out, void* grad_in, int n_frames, float step_db,
                                float floor_db, void* stream);

/* EXTENSION (stand-in for the reference's rubberband-based TimeStretch / PitchShift, scripts/attacks.py:208-252; the
 * binary is absent, parity with it unpinned): phase vocoder on one-sided spectra [frames][AWARE_FULL_STRIDE] complex64.
 * Output frame t of clip c sits at input position t*rate: linear magnitude interpolation, phase accumulated from the
 * wrapped per-bin phase increments (f64).  frame_off_* are device arrays of B+1 frame offsets; the caller sizes
 * the output as ceil(T_c / rate) frames per clip.  Used as aware_stft -> aware_phase_vocoder -> aware_istft. */
int aware_phase_vocoder(const void* spec_in, const int* frame_off_in, void* spec_out, const int* frame_off_out, int B,
                        double rate, void* stream);

/* ---- quality metric ----------------------------------------------------------------------------------
 * SNR.__call__ (src/AWARE/metrics/audio.py:68-89) per clip: 10 log10(mean(output^2) / mean((output - target)^2))
 * over lengths[c] samples (the caller passes the common length, :82-84), +inf when the clips are identical;
 * f64 accumulation in a fixed order.  Offsets are float offsets of clip c in the two signal arrays. */
int aware_snr(const float* output, const int* out_offsets, const float* target, const int* tgt_offsets,
              const int* lengths, int B, double* snr_db, void* stream);

/* STOI (short-time objective intelligibility, Taal et al. 2011) per clip pair, what STOI.__call__ (metrics/audio.py:42-64)
 * obtains from pystoi: the function aware_amd/metrics/audio.py::stoi restates on the host (parity with pystoi itself
 * unpinned), for two ragged batches ALREADY AT 10 kHz.  Per clip: frames of 256 samples every 128 (a frame that would end
 * exactly at n is not taken; n <= 256 gives none), energies of the CLEAN signal's windowed frames, frames within 40 dB of
 * the loudest kept (both signals use the clean signal's list), overlap-add of the kept frames and re-framing (K kept frames
 * give K - 1), second window, 512-point FFT of the frame zero-padded at its end, 15 third-octave bands from 150 Hz,
 * segments of 30 frames: normalisation and clipping of the processed band (-15 dB SDR), correlation, mean over segments and
 * bands.  Fewer than 30 re-framed frames: exactly 1e-5.  Frames, FFT and band sums are f32; energies are compared and the
 * segment statistics are computed in f64; every reduction has a fixed order inside one clip (no atomics), so a clip's score
 * depends neither on its neighbours nor on the run.
 * The plan holds the FFT twiddles, the window and the band edges on the device (no process-global state); it may be shared
 * by concurrent calls.  aware_stoi_band_edges copies the 15 band edges (bins lo <= k < hi) to host arrays; plan may be NULL
 * (the edges are constants).  aware_stoi_frames: first-stage frames of a clip of n samples.
 * aware_stoi_workspace_bytes: bytes for B clips, the longest of max_len samples, total_len samples in all (the sum of the
 * common lengths), with every frame kept.  aware_stoi: clean / proc dev f32, clip c at float offset clean_off[c] /
 * proc_off[c] (dev int [B]), n dev int [B] the common length of clip c (<= max_len, their sum <= total_len); out dev f64
 * [B]; kept_out dev int [B] or NULL receives K_c.  Five launches on `stream`, no allocation, no synchronisation, no copy to
 * the host.  AWARE_E_BADARG: a null argument, B < 1 or > 65535, total_len outside [max_len, B * max_len];
 * AWARE_E_WORKSPACE: workspace_bytes below aware_stoi_workspace_bytes. */
int aware_stoi_create(aware_stoi_plan** out);
void aware_stoi_destroy(aware_stoi_plan* plan);
int aware_stoi_band_edges(const aware_stoi_plan* plan, int* lo, int* hi);
int aware_stoi_frames(int n);
size_t aware_stoi_workspace_bytes(int B, int max_len, long long total_len);
int aware_stoi(const aware_stoi_plan* plan, const float* clean, const int* clean_off, const float* proc,
               const int* proc_off, const int* n, int B, int max_len, long long total_len, double* out, int* kept_out,
               void* workspace, size_t workspace_bytes, void* stream);

/* ---- attack-aware embedding (EXTENSION, parity unpinned: the reference optimises against the clean synthesis only) -------
 * A chain of up to four attacks applied to the normalised synthesis inside every loop iteration, so that the optimiser sees
 * the attacked signal: for clip b (output length Ny_b) at optimiser step s (the device step counter, aware_embed_buffer 8,
 * before the iteration advances it; aware_embed_gradient evaluates the current value), seed_b = seeds[b]:
 *   x = N(N(y)),  N(v) = v / (max|v| + 1e-8),  y the raw synthesis (buffer 9)
 *   entry j:  r = philox4x32_10(counter (0, s, 1 + j, 1), key (seed_b, 0x5EED));  on = (r[0] + 0.5) / 2^32 < prob
 *     AWARE_LOOP_SAMPLE_SUPPRESSION, param = samples k:  start = (r[1] * (Ny_b - k)) >> 32;  on: x[start : start + k] = 0
 *     AWARE_LOOP_GAUSSIAN_NOISE, param = snr_db:  sigma = sqrt(mean(x^2) / 10^(snr_db / 10)) of the current x, a CONSTANT
 *       in the backward pass;  on: x += sigma * eps, eps_i from philox4x32_10((i / 4, s, 0, j), (seed_b, 0x5EED)) through
 *       Box-Muller with the lane pairing of aware_gaussian_noise (at s = 0, j = 0 the same noise)
 *   z = x (buffer 12); the loop's analysis (two normalisers, STFT, band magnitudes) runs on z instead of y.
 * loss[] and best_loss[] are those of the attacked forward; the backward pass is the exact adjoint with sigma detached;
 * aware_embed_finish is unchanged (the clean synthesis of the best coefficients).  Works with every loss, optimiser, conv
 * pipe, read-out, dsp_path, mel form, band layout and batch shape; the step is read from device memory, so the recorded
 * graphs replay with fresh draws.
 * To be called after aware_embed_create and before the first aware_embed_iterate (later: AWARE_E_BADARG); n_attacks = 0
 * clears the chain (workspace and seeds may then be NULL).  seeds: HOST uint32 [B].  workspace: device,
 * >= aware_embed_loop_attack_workspace_bytes(batch, n_attacks) bytes, 256-byte aligned, alive as long as the handle.
 * AWARE_E_BADARG: unknown kind, n_attacks outside 0..4, prob outside [0, 1], non-finite snr_db, k < 1 or not an integer;
 * AWARE_E_UNSUPPORTED: k >= Ny_b for some clip; AWARE_E_WORKSPACE: workspace too small.  Added without a version step:
 * callers detect the feature by symbol. */
#define AWARE_LOOP_GAUSSIAN_NOISE 0      /* param = snr_db */
#define AWARE_LOOP_SAMPLE_SUPPRESSION 1  /* param = samples k (the host converts seconds * sample_rate) */
typedef struct aware_loop_attack { int kind; float param; float prob; } aware_loop_attack;
size_t aware_embed_loop_attack_workspace_bytes(const aware_batch* batch, int n_attacks);
int aware_embed_set_loop_attacks(aware_embed* e, const aware_loop_attack* attacks, int n_attacks, const uint32_t* seeds,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* ---- reverberation inside the loop and as an attack (EXTENSION, parity unpinned: the reference has neither) ---------------
 * The two entry points above keep their behaviour (kind 2 stays AWARE_E_BADARG there).  The _ex pair takes entries with four
 * parameters and, besides kinds 0 and 1 (param[0] as above; the same launches and results as through the old call), accepts
 *   AWARE_LOOP_REVERBERATION, param = { n_lo, n_hi, drr_db }: with r the entry's draw as above and
 *     n_h = n_lo + ((r[2] * (n_hi - n_lo + 1)) >> 32) taps,
 *     t_i = eps_i * exp(-ln(1000) * i / n_h) for 1 <= i < n_h, eps_i the standard normals of philox4x32_10 counter
 *       (i / 4, s, 8, j), key (seed_b, 0x5EED), paired through Box-Muller as the noise pairs them,
 *     h_0 = 10^(drr_db / 20) * sqrt(sum t_i^2),  h_i = t_i,
 *   on: x = (h * x)[0 : Ny_b], causal and truncated; h is a CONSTANT in the backward pass, which is the correlation
 *   gx[i] = sum_k h_k gy[i + k].  A noise entry behind it takes its sigma from the convolved signal.  At most one per chain.
 * The convolution is overlap-save on 4096-point transforms (blocks of 2048 output samples, the response in up to four
 * partitions of 2048 taps); a clip whose entry does not fire is copied, and a clip on which no entry of such a chain fires
 * at a step leaves the bits of the loop without a chain (its maxima are taken as 1, so the normalisers of z are the identity).  aware_embed_buffer 13: the responses of the last
 * forward pass, dev f32 [B][8192], zero beyond n_h (the unit impulse where the entry did not fire).
 * AWARE_E_BADARG of the _ex setter, besides those above: two reverberations, n_lo < 2, n_hi > 8192, n_lo > n_hi, a length
 * that is not an integer, a non-finite drr_db.  Added without a version step: callers detect the feature by symbol. */
#define AWARE_LOOP_REVERBERATION 2       /* param = n_lo, n_hi (taps; the host converts rt60 * sample_rate), drr_db */
typedef struct aware_loop_attack_ex { int kind; float prob; float param[4]; } aware_loop_attack_ex;
size_t aware_embed_loop_attack_workspace_bytes_ex(const aware_batch* batch, const aware_loop_attack_ex* attacks, int n_attacks);
int aware_embed_set_loop_attacks_ex(aware_embed* e, const aware_loop_attack_ex* attacks, int n_attacks, const uint32_t* seeds,
                                    void* workspace, size_t workspace_bytes, void* stream);
/* The same convolution alone, on a ragged batch: clip b is len[b] floats at float offset off[b] of in and out (dev int [B],
 * len[b] <= max_len), its response h[b * h_stride ...] with nh[b] taps (dev int [B]; at most h_stride <= 8192 are used;
 * nh[b] <= 0 copies the clip).  adjoint 0: out = (h * in)[0 : len];  1: out[i] = sum_k h[k] in[i + k].  out may be in.
 * workspace: device, 256-byte aligned, >= aware_convolve_workspace_bytes with nh_max >= h_stride (0: an argument out of
 * range; total_len is the sum of the lengths and only checked against [max_len, B * max_len]).  Three launches and one
 * 25 KB upload of twiddles on `stream`.  AWARE_E_BADARG: a null argument, B < 1 or > 65535, h_stride outside 1..8192;
 * AWARE_E_WORKSPACE: workspace too small. */
size_t aware_convolve_workspace_bytes(int B, int max_len, long long total_len, int nh_max);
int aware_convolve(const float* in, const int* off, const int* len, int B, int max_len, const float* h, int h_stride,
                   const int* nh, int adjoint, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* The response the loop draws for seeds[b] (dev uint32 [B]) at optimiser step `step`, chain entry `entry`, with prob 1:
 * h dev f32 [B][h_stride] (h_stride >= n_hi, zero beyond n_h), nh dev int [B].  AWARE_E_BADARG: a null argument,
 * n_lo < 2, n_hi > 8192, n_lo > n_hi, h_stride < n_hi, entry outside 0..3, a non-finite drr_db. */
int aware_reverb_ir(const uint32_t* seeds, int B, int step, int entry, int n_lo, int n_hi, float drr_db, float* h,
                    int h_stride, int* nh, void* stream);

/* ---- speed change inside the loop and as an attack (EXTENSION, parity unpinned: the reference has neither) ----------------
 * The _ex pair also accepts (the older entry point keeps refusing every kind above 1)
 *   AWARE_LOOP_SPEED_CHANGE, param = { m_lo, m_hi }: with r the entry's draw as above,
 *     m = m_lo + ((r[3] * (m_hi - m_lo + 1)) >> 32),  R = 65536 + m: the clip is played at R / 65536 of its speed (uniform in
 *     that ratio, not in cents; the host converts cents: m_lo = ceil(65536 (2^(lo / 1200) - 1)), m_hi = floor(...));
 *     p_i = i * R as a 64-bit integer in 16.16 fixed point, i0 = p_i >> 16, f = (p_i & 0xFFFF) / 65536,
 *   on: z[i] = w_-1(f) x[i0 - 1] + w_0(f) x[i0] + w_1(f) x[i0 + 1] + w_2(f) x[i0 + 2] for i < Ny_b, x read as zero outside
 *   [0, Ny_b), z[i] = 0 where p_i > (Ny_b - 1) << 16, with the Catmull-Rom weights w_-1 = ((-f + 2) f - 1) f / 2,
 *   w_0 = ((3 f - 5) f^2 + 2) / 2, w_1 = ((-3 f + 4) f + 1) f / 2, w_2 = (f - 1) f^2 / 2.  The clip keeps its length: a faster
 *   one ends in zeros, a slower one is truncated.  m = 0 is the identity.  R is a CONSTANT in the backward pass, which is
 *   gx[j] = sum over ascending i of w_{j - i0(i)}(f_i) gy[i] (no atomics).  A noise entry behind it takes its sigma from the
 *   resampled signal; a clip on which no entry of such a chain fires at a step leaves the bits of the loop without a chain.
 * AWARE_E_BADARG of the _ex setter, besides those above: a value that is not an integer, m_lo > m_hi, m_lo < -13520 or
 * m_hi > 17034 (what -+400 cents give), a second speed change, a speed change together with a reverberation.
 * aware_embed_loop_attack_workspace_bytes_ex grows by one signal for such a chain.  Added without a version step. */
#define AWARE_LOOP_SPEED_CHANGE 3        /* param = m_lo, m_hi (the host converts cents) */
/* The same operator alone, on a ragged batch: clip b of the x side is in_len[b] floats at float offset in_off[b], of the z
 * side out_len[b] floats at out_off[b] (dev int [B], any offsets, every length <= max_len <= 2^30), m dev int [B].
 * adjoint 0: `in` holds x and `out` receives z[0 : out_len[b]] (out_len = in_len keeps the geometry as the loop does;
 * ((in_len - 1) << 16) / R + 1 is the whole clip at its new speed).  adjoint 1: `in` holds gy with the lengths and offsets of
 * the z side (out_off, out_len) and `out` receives gx with those of the x side (in_off, in_len).  in and out are distinct
 * buffers.  One launch on `stream`.  AWARE_E_BADARG: a null argument, in == out, B < 1 or > 65535, max_len < 1 or > 2^30,
 * adjoint outside 0..1 (checked before anything is launched); the m[b] are taken as they are. */
int aware_speed_change(const float* in, const int* in_off, const int* in_len, float* out, const int* out_off,
                       const int* out_len, int B, int max_len, const int* m, int adjoint, void* stream);

/* ---- time stretch inside the loop and as an attack (EXTENSION, parity unpinned: the reference's is rubberband) ------------
 * The _ex pair also accepts (the older entry point keeps refusing every kind above 1)
 *   AWARE_LOOP_TIME_STRETCH, param = { m_lo, m_hi }: with r the entry's draw as above,
 *     m = m_lo + ((r[3] * (m_hi - m_lo + 1)) >> 32),  Q = 65536 + m: the clip's duration is divided by Q / 65536 at its own
 *     pitch (above 1: faster and shorter; the host converts rates: m_lo = ceil(65536 (lo - 1)), m_hi = floor(65536 (hi - 1)));
 *     H = 256, N = 1024, w the periodic Hann window of N points in f32, a_t = (t H Q) >> 16 as a 64-bit signed integer with
 *     an arithmetic shift, for every integer t >= -2,
 *   on: z[n] = 1/2 sum_t w[n - t H + 512] x[n - t H + a_t] for n < Ny_b, over the at most four t with
 *   0 <= n - t H + 512 < N in ascending order, x read as zero outside [0, Ny_b).  The clip keeps its length: a faster one ends
 *   in zeros, a slower one is truncated.  m = 0 is the identity.  Q is a CONSTANT in the backward pass, which is
 *   gx[j] = 1/2 sum over ascending t of w[j - a_t + 512] gz[j - a_t + t H], 0 <= j - a_t + 512 < N (no atomics).  A noise
 *   entry behind it takes its sigma from the stretched signal; a clip on which no entry of such a chain fires at a step
 *   leaves the bits of the loop without a chain.
 *   An AWARE_LOOP_SPEED_CHANGE entry may follow the stretch DIRECTLY: the two then form one stage (stretch, then resampling;
 *   each with its own draw, so tempo and pitch move independently and a pitch shift is the diagonal).
 * AWARE_E_BADARG of the _ex setter, besides those above: a value that is not an integer, m_lo > m_hi, m_lo < -16384 or
 * m_hi > 21845 (what the rates 0.75 and 4/3 give), a second time stretch, a time stretch together with a reverberation, a
 * speed change in the same chain anywhere but directly behind the stretch.
 * aware_embed_loop_attack_workspace_bytes_ex grows by one signal for such a chain, by two for the pair; chains without the
 * kind need what they needed.  Added without a version step. */
#define AWARE_LOOP_TIME_STRETCH 4        /* param = m_lo, m_hi (the host converts rates); a pitch shift, the diagonal of
                                          * the stretch-speed pair with one draw for both, is AWARE_LOOP_PITCH_SHIFT below */
/* The same operator alone, on a ragged batch, with the argument list of aware_speed_change: clip b of the x side is in_len[b]
 * floats at float offset in_off[b], of the z side out_len[b] floats at out_off[b] (dev int [B], any offsets, every length
 * <= max_len <= 2^30), m dev int [B].  adjoint 0: `in` holds x and `out` receives z[0 : out_len[b]] (out_len = in_len keeps
 * the geometry as the loop does; ((in_len - 1) << 16) / Q + 1 is the whole clip at its new duration).  adjoint 1: `in` holds
 * gz with the lengths and offsets of the z side (out_off, out_len) and `out` receives gx with those of the x side (in_off,
 * in_len).  in and out are distinct buffers.  One launch on `stream`; the first call on a device uploads the window table
 * (4 KiB, synchronously: not inside a stream capture).  AWARE_E_BADARG: a null argument, in == out, B < 1 or > 65535,
 * max_len < 1 or > 2^30, adjoint outside 0..1 (checked before anything is launched); a clip whose m[b] lies outside
 * -16384..21845 is copied as with m = 0. */
int aware_stretch_ola(const float* in, const int* in_off, const int* in_len, float* out, const int* out_off,
                      const int* out_len, int B, int max_len, const int* m, int adjoint, void* stream);

/* ---- pitch shift inside the loop and as an attack (EXTENSION, parity unpinned: the reference's is a library call) ------------
 * The _ex pair also accepts (the older entry point keeps refusing every kind above 1)
 *   AWARE_LOOP_PITCH_SHIFT, param = { m_lo, m_hi }, the speed offsets of AWARE_LOOP_SPEED_CHANGE: with r the entry's draw,
 *     m = m_lo + ((r[3] * (m_hi - m_lo + 1)) >> 32),  R = 65536 + m: the pitch moves by the ratio R / 65536 (the host converts
 *     cents as for the speed change) and the duration stays.  The coupled rate Q = ((1 << 32) + R / 2) / R and
 *     L_u = ((Ny_b - 1) << 16) / Q + 1 in 64-bit integers;
 *   on: u = the AWARE_LOOP_TIME_STRETCH operator at Q on x, L_u samples long (its true stretched length) and zero outside;
 *   z = the AWARE_LOOP_SPEED_CHANGE operator at R on u, Ny_b samples long.  One fused launch: u is never in memory.  m = 0 is
 *   the identity.  R and Q are CONSTANTS in the backward pass, which is the exact transpose in gather form (the resampling's
 *   into gu over ascending i, then the stretch's over ascending t; no atomics).  Entries in front of it and behind it behave as
 *   around a lone speed change, and a clip on which no entry fires at a step leaves the bits of the loop without a chain.
 * AWARE_E_BADARG of the _ex setter, besides those above: a value that is not an integer, m_lo > m_hi, m_lo < -13520 or
 * m_hi > 17034, a second pitch shift, a pitch shift together with a reverberation, a speed change or a time stretch.
 * aware_embed_loop_attack_workspace_bytes_ex for a chain with the kind is that of the same chain with a speed change in its
 * place; chains without the kind need what they needed.  Added without a version step. */
#define AWARE_LOOP_PITCH_SHIFT 5         /* param = m_lo, m_hi (the host converts cents) */
/* The same operator alone, on a ragged batch, with the argument list and the conventions of aware_speed_change and
 * aware_stretch_ola (x side: in_off / in_len, z side: out_off / out_len; adjoint 1 reads gz on the z side and writes gx on the
 * x side; the window table is uploaded on the first call on a device).  AWARE_E_BADARG as aware_stretch_ola; a clip whose m[b]
 * lies outside -13520..17034 is copied as with m = 0. */
int aware_pitch_shift_ola(const float* in, const int* in_off, const int* in_len, float* out, const int* out_off,
                          const int* out_len, int B, int max_len, const int* m, int adjoint, void* stream);

/* ---- phase vocoder inside the loop (EXTENSION, parity unpinned: the reference's TimeStretch / PitchShift are library calls) ---
 * The _ex pair also accepts (the older entry point keeps refusing every kind above 1)
 *   AWARE_LOOP_PHASE_VOCODER, param = { mq_lo, mq_hi, m_lo, m_hi }: the stretch offsets of AWARE_LOOP_TIME_STRETCH and the
 *     speed offsets of AWARE_LOOP_SPEED_CHANGE (the host converts rates and cents).  A mode is ABSENT where its lo > hi (the
 *     host passes 0, -1); at least one is present.  With r the entry's draw: stretch mode where only the stretch range is
 *     present, or both are and r[2] < 2^31; pitch mode otherwise.
 *     stretch mode: mq = mq_lo + ((r[3] * (mq_hi - mq_lo + 1)) >> 32), m = 0;
 *     pitch mode:   m = m_lo + ((r[3] * (m_hi - m_lo + 1)) >> 32), R = 65536 + m, mq = ((1 << 32) + R / 2) / R - 65536.
 *   Q = 65536 + mq.  on: S = STFT(x) (the loop's geometry, T_b frames); for t < T_b: p = t Q (64-bit), i = p >> 16,
 *   al = (p & 0xFFFF) / 65536; Y[t] = ((1 - al) |S[i]| + al |S[i + 1]|) P[t] with S[T_b] := 0 and Y[t] = 0 where i >= T_b;
 *   P[0] = u(S[0]), P[t + 1] = P[t] u(S[i + 1]) conj(u(S[i])), u(c) = c / |c| and u(c) = 1 where both parts of c are zero;
 *   z = the AWARE_LOOP_SPEED_CHANGE operator at m on iSTFT(Y), Ny_b samples long.  mq = 0 is the identity.  P, Q and m are
 *   CONSTANTS in the backward pass (no phase gradients); d|c|/dc is 0 at a zero cell.  Entries in front of it and behind it
 *   behave as around a lone speed change; a clip on which the entry does not fire keeps its bits through the stage, and one
 *   on which no entry fires leaves the bits of the loop without a chain.
 * AWARE_E_BADARG of the _ex setter, besides those above: a value that is not an integer, both modes absent, a present
 * stretch range outside -16384..21845, a present speed range outside -13520..17034, a second phase vocoder, a phase vocoder
 * together with a reverberation, a speed change, a time stretch or a pitch shift (in either order).
 * aware_embed_loop_attack_workspace_bytes_ex for a chain with the kind is that of the same chain with a speed change in its
 * place plus two spectra of [total frames][520] complex values (each rounded up to 256 bytes); chains without the kind need
 * what they needed.  Added without a version step. */
#define AWARE_LOOP_PHASE_VOCODER 6       /* param = mq_lo, mq_hi, m_lo, m_hi; lo > hi: the mode is absent */
/* The frames' two kernels alone.  spec, out, grad_out, grad_spec: [frame_off[B]][520] complex float rows as aware_stft writes
 * them, clip b's T_b = frame_off[b + 1] - frame_off[b] rows at row frame_off[b] (dev int [B + 1]); mq dev int [B], a value
 * outside -16384..21845 is read as 0, which copies the clip's rows.  aware_pv_frames: out = Y from spec = S (never the same
 * buffer).  aware_pv_frames_bwd: grad_spec = gS from spec = S and grad_out = dL/dY; grad_spec may be spec, never grad_out.
 * AWARE_E_BADARG: a null pointer, B outside 1..65535, buffers that may not coincide. */
int aware_pv_frames(const void* spec, const int* frame_off, int B, const int* mq, void* out, void* stream);
int aware_pv_frames_bwd(const void* spec, const void* grad_out, const int* frame_off, int B, const int* mq, void* grad_spec,
                        void* stream);

/* ---- sample deletion inside the loop (EXTENSION, parity unpinned: the reference's Cropout / DeleteSamples are post-hoc) --------
 * The _ex pair also accepts (the older entry point keeps refusing every kind above 1)
 *   AWARE_LOOP_DELETE_SAMPLES, param = { k_lo, k_hi, at, 0 }: with r the entry's draw as above,
 *     k = k_lo + ((r[2] * (k_hi - k_lo + 1)) >> 32) samples are cut out,
 *     start = 0 for at = 0 (the reference's Cropout), (r[1] * (Ny_b - k)) >> 32 for at = 1 (its DeleteSamples);
 *   on: z[i] = x[i] for i < start, x[i + k] for start <= i < Ny_b - k, 0 for i >= Ny_b - k.  The clip keeps its length: the
 *   remainder moves up and zeros follow.  The backward pass is the exact adjoint in gather form: gx[i] = gz[i] for i < start,
 *   0 for start <= i < start + k, gz[i - k] for i >= start + k.  Every value is a copy.  A noise entry behind it takes its
 *   sigma from the shortened signal; a clip on which no entry of such a chain fires at a step leaves the bits of the loop
 *   without a chain.
 * AWARE_E_BADARG of the _ex setter, besides those above: a value that is not an integer, k_lo < 1, k_lo > k_hi, at other than
 * 0 or 1, a second sample deletion, a sample deletion together with a reverberation, a speed change, a time stretch, a pitch
 * shift or a phase vocoder (in either order).  AWARE_E_UNSUPPORTED: k_hi >= Ny_b for some clip, as for a sample suppression
 * that is too long.  aware_embed_loop_attack_workspace_bytes_ex for a chain with the kind is that of the same chain with a
 * speed change in its place; chains without the kind need what they needed.  aware_embed_buffer gains no index.  Added
 * without a version step: callers detect the addition by symbol. */
#define AWARE_LOOP_DELETE_SAMPLES 7      /* param = k_lo, k_hi, at (0: start, 1: anywhere), 0 */
/* The same operator alone, on a ragged batch: clip b is len[b] floats at float offset off[b] of `in` and of `out` (dev int
 * [B], any offsets, every length <= max_len <= 2^30); start and k dev int [B], read as k = min(max(k, 0), len) and
 * start = min(max(start, 0), len - k); k = 0 is the identity.  adjoint 0: `in` holds x and `out` receives z.  adjoint 1: `in`
 * holds gz and `out` receives gx.  in and out are distinct buffers.  One launch on `stream`.  AWARE_E_BADARG: a null
 * argument, in == out, B < 1 or > 65535, max_len < 1 or > 2^30, adjoint outside 0..1 (checked before anything is launched). */
int aware_delete_samples(const float* in, const int* off, const int* len, int B, int max_len, const int* start, const int* k,
                         float* out, int adjoint, void* stream);

/* ---- gain envelope inside the loop and alone (EXTENSION, parity unpinned: the reference has neither) -----------------------
 * The _ex pair and the mixture's setter also accept (the older entry point keeps refusing every kind above 1)
 *   AWARE_LOOP_GAIN_ENVELOPE, param = { P_lo, P_hi, floor, 0 }: a gain that moves over time, piecewise linear between random
 *     breakpoints (a fade, ducking, tremolo, an AGC riding the level).  With r the entry's draw as above,
 *     P = P_lo + ((r[2] * (P_hi - P_lo + 1)) >> 32) samples between breakpoints (the host converts seconds),
 *     ph = (r[1] * P) >> 32;  breakpoint k >= 0: w_k = philox4x32_10((k / 4, s, 16 + j, 0), (seed_b, 0x5EED))[k % 4],
 *     u_k = (w_k >> 8) * 2^-24, g_k = floor + (1 - floor) * u_k in f32;  at sample i: pos = i + ph, k = pos / P,
 *     f = (float)(pos - k * P) / (float)P, g(i) = g_k + f * (g_{k+1} - g_k);
 *   on: z[i] = g(i) * x[i].  P may exceed Ny_b: the clip then sees one ramp.  g is a CONSTANT in the backward pass, which is
 *   the same operator: gx[i] = g(i) * gz[i].  The kind is ELEMENT-WISE, as kinds 0 and 1 are: it runs inside the stage kernels,
 *   never splits a chain, may stand any number of times (up to the chain's four entries) in front of and behind a splitting
 *   entry and in every chain of a mixture, and a noise entry behind it takes its sigma from the enveloped signal.  The device
 *   evaluates f with a reciprocal and a fused multiply-add: g is within 1e-6 of the formula above.
 * AWARE_E_BADARG of the _ex setter, besides those above: a period that is not an integer, P_lo < 64, P_lo > P_hi,
 * P_hi > 1048576, floor outside [0, 1) or not finite.  aware_embed_loop_attack_workspace_bytes_ex for a chain with the kind is
 * that of the same chain with a Gaussian noise in its place: no new workspace.  Added without a version step: callers detect
 * the addition by symbol. */
#define AWARE_LOOP_GAIN_ENVELOPE 8       /* param = P_lo, P_hi (samples; the host converts seconds), floor, 0 */
/* The same operator alone, on a ragged batch, always on: clip b is len[b] floats at float offset off[b] of `in` and of `out`
 * (dev int [B], any offsets, every length <= max_len <= 2^30); seeds dev uint32 [B]; the draw is that of chain entry `entry`
 * (0..3) at optimiser step `step` (>= 0).  out[i] = g(i) * in[i]; out may be in.  gains: NULL, or dev float with the layout of
 * `out`, receives g itself.  The operator is its own adjoint.  One launch on `stream`.  AWARE_E_BADARG: a null argument (gains
 * apart), B < 1 or > 65535, max_len < 1 or > 2^30, step < 0, entry outside 0..3, the periods or the floor as above (checked
 * before anything is launched). */
int aware_gain_envelope(const float* in, const int* off, const int* len, int B, int max_len, const uint32_t* seeds, int step,
                        int entry, int p_lo, int p_hi, float floor, float* out, float* gains, void* stream);

/* ---- band filter inside the loop and alone (EXTENSION, parity unpinned: the reference's LowPassFilter, HighPassFilter and
 * RandomBandstop are post-hoc IIR attacks) ------------------------------------------------------------------------------------
 * The _ex pair and the mixture's setter also accept (the older entry point keeps refusing every kind above 1)
 *   AWARE_LOOP_BAND_FILTER, param = { mask, c_lo, c_hi, w_min }: a frequency-selective channel, a zero-phase windowed-sinc FIR
 *     of 255 taps.  Frequencies are integers c = round(65536 * f / sample_rate), in units of 1 / 65536 cycle per sample
 *     (Nyquist is 32768; the host converts Hz).  mask: bit 1 lowpass, 2 highpass, 4 bandpass, 8 bandstop, the responses drawn
 *     from.  With r the entry's draw as above,
 *     e1 = c_lo + ((r[1] * (c_hi - c_lo + 1)) >> 32), e2 the same from r[2],
 *     response = the ((r[3] * popcount(mask)) >> 32)-th set bit of mask, counted from the lowest;
 *     lowpass and highpass: c1 = e1;  band responses: c1 = min(e1, e2), c2 = max(e1, e2), and c2 = c1 + w_min if c2 - c1 < w_min;
 *     w[k] = 0.54 + 0.46 * cos(pi * k / 127), lp_c[0] = c / 32768,
 *     lp_c[k] = w[k] * sin(2 * pi * ((c * |k|) mod 65536) / 65536) / (pi * |k|), k = -127..127, delta the unit impulse at 0;
 *     h = lp_c1 (lowpass), delta - lp_c1 (highpass), lp_c2 - lp_c1 (bandpass), delta - (lp_c2 - lp_c1) (bandstop);
 *   on: z[i] = sum_k h[k] * x[i - k], 0 <= i < Ny_b, x zero outside the clip.  The clip keeps its length and there is no delay.
 *   h is symmetric and the extension is by zeros, so the backward pass is the same operator on the gradient with the same
 *   draw.  The kind SPLITS a chain as kinds 2 to 7 do: at most one per chain, none of them beside it, element-wise entries on
 *   either side (noise in front of it is coloured noise; noise behind it takes its sigma from the filtered signal); a clip on
 *   which no entry of such a chain fires at a step leaves the bits of the loop without a chain.  The device builds the taps in
 *   f32 with the sine's argument inside one turn: they are within 1e-6 of the formula above.
 * AWARE_E_BADARG of the _ex setter, besides those above: a value that is not an integer, mask outside 1..15, c_lo < 1,
 * c_lo > c_hi, w_min < 1, c_hi + w_min > 32767, a second band filter, a band filter together with any of kinds 2 to 7 (in
 * either order).  aware_embed_loop_attack_workspace_bytes_ex for a chain with the kind is that of the same chain with a sample
 * deletion in its place: no private workspace.  aware_embed_buffer gains no index.  Added without a version step: callers
 * detect the addition by symbol. */
#define AWARE_LOOP_BAND_FILTER 9         /* param = mask, c_lo, c_hi, w_min (1 / 65536 cycle per sample; the host converts Hz) */
/* The same operator alone, on a ragged batch, always on: clip b is len[b] floats at float offset off[b] of `in` and of `out`
 * (dev int [B], any offsets, every length <= max_len <= 2^30); response dev int [B], each one of 1, 2, 4, 8 (the lowest set bit
 * of the low four is read; none: a copy); c1, c2 dev int [B], read clamped to 0..32767, c2 by the band responses only.  in and
 * out are distinct buffers.  taps: NULL, or dev float [B][256]: receives clip b's taps, tap k at index k + 127, zero at 255.
 * The operator is its own adjoint.  One launch on `stream`.  AWARE_E_BADARG: a null argument (taps apart), in == out, B < 1 or
 * > 65535, max_len < 1 or > 2^30 (checked before anything is launched). */
int aware_band_filter(const float* in, const int* off, const int* len, int B, int max_len, const int* response, const int* c1,
                      const int* c2, float* out, float* taps, void* stream);

/* ---- tiled excerpt inside the loop and alone (EXTENSION, parity unpinned: the reference's Cropout is a post-hoc attack) ------
 * The _ex pair and the mixture's setter also accept (the older entry point keeps refusing every kind above 1)
 *   AWARE_LOOP_EXCERPT, param = { L_lo, L_hi, 0, 0 }: what a detector sees of an excerpt of the clip.  The excerpt
 *     [start, start + L) is repeated periodically until it fills the clip, so the clip keeps its length and every norm and mean
 *     along time sees the excerpt's own statistics.  With r the entry's draw as above,
 *     L = min(L_lo + ((r[2] * (L_hi - L_lo + 1)) >> 32), Ny), and L = Ny where the entry does not fire;
 *     start = (r[1] * (Ny - L + 1)) >> 32, so 0 <= start <= Ny - L;
 *     forward  z[i] = x[start + (i mod L)], 0 <= i < Ny: every value is a copy;
 *     adjoint  gx[i] = sum_m gz[(i - start) + m * L] for start <= i < start + L, over m = 0, 1, .. while the index is below Ny,
 *     in f32 with m ascending (the first term is copied, every further one is one rounded addition), and +0.0 outside.
 *   An excerpt as long as the clip is the identity in both directions, bit for bit; a clip shorter than L_lo is therefore left
 *   alone and not refused.
 * AWARE_E_BADARG of the _ex setter, besides those above: a value that is not an integer, L_lo < 1024, L_lo > L_hi,
 * L_hi > 2147483520, param[2] or param[3] not 0, a second excerpt, an excerpt together with any of kinds 2 to 7 and 9 (in
 * either order).  aware_embed_loop_attack_workspace_bytes_ex for a chain with the kind is that of the same chain with a sample
 * deletion in its place: no private workspace.  aware_embed_buffer gains no index.  Added without a version step: callers
 * detect the addition by symbol. */
#define AWARE_LOOP_EXCERPT 10            /* param = L_lo, L_hi, 0, 0 (samples) */
/* The same operator alone, on a ragged batch: clip b is len[b] floats at float offset off[b] of `in` and of `out` (dev int
 * [B], any offsets, every length <= max_len <= 2^30); start and length dev int [B], read as length = min(max(length, 1), len)
 * and start = min(max(start, 0), len - length); length = len is the identity.  adjoint 0: `in` holds x and `out` receives z.
 * adjoint 1: `in` holds gz and `out` receives gx.  in and out are distinct buffers.  One launch on `stream`.  AWARE_E_BADARG:
 * a null argument, in == out, B < 1 or > 65535, max_len < 1 or > 2^30, adjoint outside 0..1 (checked before anything is
 * launched). */
int aware_excerpt_tile(const float* in, const int* off, const int* len, int B, int max_len, const int* start, const int* length,
                       float* out, int adjoint, void* stream);

/* ---- time warp inside the loop and alone (EXTENSION, parity unpinned: the reference has neither) -----------------------------
 * The _ex pair and the mixture's setter also accept (the older entry point keeps refusing every kind above 1)
 *   AWARE_LOOP_TIME_WARP, param = { e_lo, e_hi, D, 0 }: the clip resampled at a rate that is piecewise linear in time between
 *     drawn breakpoints 2^e samples apart: wow and flutter, a drifting sample clock.  With r the entry's draw as above,
 *     e = e_lo + ((r[2] * (e_hi - e_lo + 1)) >> 32), P = 2^e, ph = (r[1] * P) >> 32;
 *     w_k = philox4x32_10((k / 4, s, 20 + j, 0), (seed_b, 0x5EED))[k % 4], m_k = -D + ((w_k * (2 D + 1)) >> 32),
 *     R_k = 65536 + m_k, for breakpoint k >= 0;
 *     in signed 64-bit integers with arithmetic shifts: A(0) = 0, A(k + 1) = A(k) + P R_k + (((R_{k+1} - R_k) P) >> 1);
 *     Pos(u) = A(k) + t R_k + (((R_{k+1} - R_k) t t) >> (e + 1)) with k = u >> e, t = u & (P - 1);
 *     p_i = Pos(i + ph) - Pos(ph), i0 = p_i >> 16, f = (p_i & 0xFFFF) / 65536;
 *     forward  z[i] = the Catmull-Rom tap of the speed change at (i0, f), x zero outside [0, Ny); 0 where p_i > (Ny - 1) << 16;
 *     adjoint  gx[j] = sum over ascending i of w_{j - i0(i)}(f_i) gz[i], gathered in one fixed order.
 *   The clip keeps its length.  An entry that does not fire copies the clip; the rates are not differentiated.
 * AWARE_E_BADARG of the _ex setter, besides those above: a value that is not an integer, e_lo < 8, e_lo > e_hi, e_hi > 20,
 * D < 1, D > 6553, param[3] not 0, a second time warp, a time warp together with any of kinds 2 to 7, 9 and 10 (in either
 * order).  aware_embed_loop_attack_workspace_bytes_ex for a chain with the kind is that of the same chain with a sample
 * deletion in its place, and behind it, each at the next 256-byte boundary, int [B][K] and long long [B][K] with
 * K = ((Ny_max + 2^e_lo - 1) >> e_lo) + 2: R_k and A(k) of the last forward pass, which the backward pass reads.
 * aware_embed_buffer gains no index.  Added without a version step: callers detect the addition by symbol. */
#define AWARE_LOOP_TIME_WARP 11          /* param = e_lo, e_hi, D, 0 */
/* The same operator alone, on a ragged batch: clip b is len[b] floats at float offset off[b] of `in` and of `out` (dev int
 * [B], any offsets, every length <= max_len <= 2^30); e and ph dev int [B], read as e = min(max(e, 8), 20) and
 * ph = min(max(ph, 0), 2^e - 1); rates dev int [B][stride], m_k of clip b at rates[b * stride + k], each read as
 * min(max(m, -6553), 6553), and an index from `stride` on reads the last one (the caller provides
 * stride >= ((len[b] + 2^e[b] - 1) >> e[b]) + 2 for every clip); table_r dev int [B][stride] and table_a dev long long
 * [B][stride] receive R_k and A(k) (adjoint 0) and are read (adjoint 1: the tables of the forward call).  adjoint 0: `in`
 * holds x and `out` receives z.  adjoint 1: `in` holds gz and `out` receives gx.  in and out are distinct buffers.  At most two
 * launches on `stream`.  AWARE_E_BADARG: a null argument, in == out, B < 1 or > 65535, max_len < 1 or > 2^30, stride < 3,
 * adjoint outside 0..1 (checked before anything is launched). */
int aware_time_warp(const float* in, const int* off, const int* len, int B, int max_len, const int* e, const int* ph,
                    const int* rates, int stride, int* table_r, long long* table_a, float* out, int adjoint, void* stream);

/* ---- frequency shift inside the loop and alone (EXTENSION, parity unpinned: the reference has neither) ----------------------
 * The _ex pair and the mixture's setter also accept (the older entry point keeps refusing every kind above 1)
 *   AWARE_LOOP_FREQUENCY_SHIFT, param = { d_lo, d_hi, 0, 0 }: single-sideband modulation, every component of the clip moved by
 *     the same number of Hz: a mistuned SSB or heterodyne link, an analogue carrier system.  Shifts are signed integers d in units
 *     of sample_rate / 2^20 Hz, |d| <= 65536 (sample_rate / 16; the host converts Hz), phases integers in units of 2^-20 turn.
 *     With r the entry's draw as above,
 *     d = d_lo + ((r[1] * (d_hi - d_lo + 1)) >> 32), p0 = r[2] >> 12;
 *     w[k] = 0.54 + 0.46 * cos(pi * k / 127), h[k] = w[k] * 2 / (pi * k) for odd k, 0 for even k, k = -127..127;
 *     (Hx)[i] = sum_k h[k] * x[i - k], x zero outside the clip;  phi_i = 2 * pi * ((p0 + i * d) mod 2^20) / 2^20;
 *     forward  z[i] = x[i] * cos(phi_i) - (Hx)[i] * sin(phi_i), 0 <= i < Ny_b: a positive d shifts upwards;
 *     adjoint  gx[j] = g[j] * cos(phi_j) + (H(g * sin(phi)))[j]: exact, because h is antisymmetric and the extension is by zeros.
 *   The clip keeps its length and there is no delay.  An entry that does not fire copies the clip; d and p0 are not
 *   differentiated.  Below about 150 Hz the 255-tap transformer leaves some of the image sideband.
 * AWARE_E_BADARG of the _ex setter, besides those above: a value that is not an integer, d_lo < -65536, d_lo > d_hi,
 * d_hi > 65536, param[2] or param[3] not 0, a second frequency shift, a frequency shift together with any of kinds 2 to 7 and 9
 * to 11 (in either order).  aware_embed_loop_attack_workspace_bytes_ex for a chain with the kind is that of the same chain with a
 * sample deletion in its place: no private workspace.  aware_embed_buffer gains no index.  Added without a version step: callers
 * detect the addition by symbol. */
#define AWARE_LOOP_FREQUENCY_SHIFT 12    /* param = d_lo, d_hi, 0, 0 (sample_rate / 2^20 Hz, signed; the host converts Hz) */
/* The same operator alone, on a ragged batch, always on: clip b is len[b] floats at float offset off[b] of `in` and of `out`
 * (dev int [B], any offsets, every length <= max_len <= 2^30); d and p0 dev int [B], p0 read modulo 2^20.  adjoint 0: `in` holds
 * x and `out` receives z.  adjoint 1: `in` holds gz and `out` receives gx.  in and out are distinct buffers.  One launch on
 * `stream`.  AWARE_E_BADARG: a null argument, in == out, B < 1 or > 65535, max_len < 1 or > 2^30, adjoint outside 0..1 (checked
 * before anything is launched). */
int aware_frequency_shift(const float* in, const int* off, const int* len, int B, int max_len, const int* d, const int* p0,
                          int adjoint, float* out, void* stream);

/* ---- attack mixtures (EXTENSION, parity unpinned: the reference has no attacks in its loop) -------------------------------
 * A handle holds one chain, and the kinds that split a chain refuse each other.  A mixture is a list of 1..8 chains, each a
 * valid chain of aware_embed_set_loop_attacks_ex with a weight; at optimiser step s clip b draws
 *     r = philox4x32_10((0, s, 12, 1), (seed_b, 0x5EED)),   T_c = min(floor((w_0 + .. + w_c) * 2^32), 2^32)
 * (the float weights summed in double), and goes through the first chain c with r[0] < T_c exactly as on a handle that holds
 * chain c alone: the same entry indices, draws, noise streams, prob gating and idle rule, forward and backward.  What the
 * weights leave of 1 is the share of steps without a chain: such a clip (choice -1) leaves the bits of the loop without a
 * chain, as an idle clip of a chain that splits does.  A mixture of one chain of weight 1 is that chain, bit for bit.
 * Calling rules as aware_embed_set_loop_attacks_ex (before the first aware_embed_iterate, else AWARE_E_BADARG); n_chains = 0
 * clears the mixture; a mixture and a plain chain replace each other.  Per chain every AWARE_E_BADARG / AWARE_E_UNSUPPORTED
 * of the _ex setter applies; besides: n_chains outside 0..8, an empty chain, a weight that is negative or not finite, a
 * weight sum above 1 + 1e-6, a SECOND chain with a reverberation (AWARE_E_BADARG), a workspace that is too small
 * (AWARE_E_WORKSPACE).  workspace: device memory, 256-byte aligned, alive as long as the handle: the buffers of a chain of
 * kinds 0/1 and one signal (if a chain has a kind that splits it) shared by all chains -- every clip belongs to one chain
 * at a step, and the kernels skip the clips of the others -- then per chain what its backward pass needs from its forward
 * pass (responses and spectra of the reverberation, the two spectra of the phase vocoder, the signal between a stretch and a
 * speed change), then int [B] choices at the next 256-byte boundary.  For one chain that is
 * aware_embed_loop_attack_workspace_bytes_ex rounded up to 256, plus 4 * B.
 * aware_embed_buffer 14: int [B], the choices of the last forward pass (NULL without a mixture); 12 as before; 13 the
 * responses of the mixture's reverberation chain (a row is refreshed at the steps its clip draws that chain; zeros before).
 * aware_loop_mixture_draw: the draw alone, for B seeds (dev) at `step`, weights on the host, choice dev int [B]; one launch.
 * Added without a version step: callers detect the addition by symbol. */
typedef struct aware_loop_chain { const aware_loop_attack_ex* attacks; int n_attacks; float weight; } aware_loop_chain;
size_t aware_embed_loop_mixture_workspace_bytes(const aware_batch* batch, const aware_loop_chain* chains, int n_chains);
int aware_embed_set_loop_mixture(aware_embed* e, const aware_loop_chain* chains, int n_chains, const uint32_t* seeds,
                                 void* workspace, size_t workspace_bytes, void* stream);
int aware_loop_mixture_draw(const uint32_t* seeds, int B, int step, const float* weights, int n_chains, int* choice,
                            void* stream);

/* ---- attack-aware embedding at any STFT geometry (EXTENSION, parity unpinned) ------------------------
 * The setters above serve the card geometry only and refuse a session on a general plan (AWARE_PLAN_GENERAL).  This one
 * serves such a session, with the kinds that do not split a chain: AWARE_LOOP_GAUSSIAN_NOISE, AWARE_LOOP_SAMPLE_SUPPRESSION
 * and AWARE_LOOP_GAIN_ENVELOPE, up to four entries in any order, parameters as aware_embed_set_loop_attacks_ex takes them.
 * The model is the card's: at optimiser step s (aware_embed_buffer 8) clip b (Ny_b = hop * (T_b - 1) samples) goes through
 *     x = N(N(yraw)),  z = chain(x) with the draws of the card route (sample i of a clip uses the counter word it uses there),
 *     a = N(N(z)),     N(v) = v / (max|v| + 1e-8)
 * and the loop's analysis reads a; the backward pass is the adjoint of exactly that, with the noise amplitude, the mask and
 * the gains as constants.  At the card geometry a general session therefore sees the very draws a card session sees with the
 * same chain and seeds.  aware_embed_iterate (eager and recorded), aware_embed_gradient (at the current step, which it does not
 * advance) and aware_embed_profile honour the chain; aware_embed_buffer 12 is z of the last forward pass, 9 stays yraw.
 * Calling rules as aware_embed_set_loop_attacks_ex: before the first aware_embed_iterate; n_attacks = 0 clears the chain, and
 * the session then launches what it launched before; seeds: host uint32 [B]; workspace: device memory, 256-byte aligned, alive
 * as long as the handle, aware_embed_general_chain_workspace_bytes large (z, and per piece of 3072 samples of every clip the
 * partial maxima, sums of squares and dot products the kernels exchange).
 * AWARE_E_BADARG: what the card's setter calls a bad argument (a null or misaligned pointer, n_attacks outside 0..4, a kind
 * outside the table, prob outside [0, 1], a parameter outside its range, a call after the first iterate).
 * AWARE_E_UNSUPPORTED: a session that is not on a general plan; a well-formed entry of any other kind; a suppression with
 * k >= Ny_b for some clip.  AWARE_E_WORKSPACE: a workspace smaller than the size function says.  The size function returns 0
 * for a card batch and for a chain that is AWARE_E_BADARG.  Added without a version step: callers detect the addition by
 * symbol. */
size_t aware_embed_general_chain_workspace_bytes(const aware_batch* batch, const aware_loop_attack_ex* attacks, int n_attacks);
int aware_embed_set_general_chain(aware_embed* e, const aware_loop_attack_ex* attacks, int n_attacks, const uint32_t* seeds,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- offset search in detection (EXTENSION, parity unpinned: the reference detects at the clip's own start only) -----------
 * The detector pools pairs of frames of hop 256, so its read-out has a period of 512 samples in where the clip starts, and a
 * clip whose first d samples are gone reads worse the nearer d mod 512 is to 256.  The host detects n views of each clip, view
 * j with a further j * (512 / n) samples dropped (one aware_detect on a batch of B * n rows with overlapping in_offsets), and
 * this entry keeps the best view per clip:
 *   values [B][n][L] f32 (clip-major), c_j = mean_l |values[b][j][l] - centre| accumulated in f32 in one fixed order,
 *   j* = the smallest j with the largest c_j;  out_values[b][0 : L] = values[b][j*], out_index[b] = j*, out_conf[b] = c_j*.
 * centre is 0.5 for a sigmoid read-out and 0 otherwise.  One wave per clip, one launch on `stream`.  AWARE_E_BADARG: a null
 * pointer, values == out_values, B outside 1..65535, n outside 1..64, L outside 1..65536, a non-finite centre. */
int aware_sync_select(const float* values, int B, int n, int L, float centre, float* out_values, int* out_index,
                      float* out_conf, void* stream);

/* ---- speed search in detection (EXTENSION, parity unpinned: the reference detects a clip as it is) -------------------------
 * A clip that was played at another speed (resampled: pitch and tempo move together) reads its bits again once it is played
 * back at the inverse speed.  The host detects n_views resampled views of each clip, m[0] = 0 first (one aware_detect on a
 * batch of B * n_views rows, times the views of the offset search where that is on), and keeps the best view per clip with
 * aware_sync_select.  This entry writes the views, all in one launch on `stream`:
 *   clip b is in_len[b] floats at float offset in_off[b] of `in` (dev int [B], any offsets); m dev int [n_views];
 *   view (b, j): R = 65536 + m[j], n_out = ((in_len[b] - 1) << 16) / R + 1 floats at out + out_off[b * n_views + j]
 *   (dev int [B * n_views], from the host: rows that start at multiples of 4 floats are stored 16 bytes at a time), equal
 *   bit for bit to aware_speed_change at m[j] with out_len = n_out; m[j] = 0 copies the clip.  max_len >= every n_out.
 *   Floats of `out` outside the rows are not written.  A view whose m[j] lies outside -13520..17034 is not written.
 * AWARE_E_BADARG, before anything is launched: a null pointer, in == out, B outside 1..65535, n_views outside 1..63,
 * max_len outside 1..2^30.  Added without a version step: callers detect the addition by symbol. */
int aware_speed_views(const float* in, const int* in_off, const int* in_len, int B, const int* m, int n_views, float* out,
                      const int* out_off, int max_len, void* stream);

/* ---- shift search in detection (EXTENSION, parity unpinned: the reference detects a clip as it is) -------------------------
 * A clip whose every component was moved by the same number of Hz (single-sideband modulation) reads its bits again once it
 * is moved back.  The host detects n_views shifted views of each clip, d[0] = 0 first (one aware_detect on a batch of
 * B * n_views rows, times the views of the offset search where that is on), and keeps the best view per clip with
 * aware_sync_select.  This entry writes the views, all in one launch on `stream`:
 *   clip b is in_len[b] floats at float offset in_off[b] of `in` (dev int [B], any offsets); d dev int [n_views], shifts in
 *   units of sample_rate / 2^20 Hz, signed, positive upwards;
 *   view (b, j): in_len[b] floats at out + out_off[b * n_views + j] (dev int [B * n_views], from the host: rows that start
 *   at multiples of 4 floats are stored 16 bytes at a time), equal bit for bit to aware_frequency_shift at d[j] with
 *   p0 = 0; d[j] = 0 gives the clip itself.  The Hilbert transform is computed once per clip and shared by its views.
 *   max_len >= every in_len[b].  Floats of `out` outside the rows are not written.  A view whose d[j] lies outside
 *   -65536..65536 is not written.
 * AWARE_E_BADARG, before anything is launched: a null pointer, in == out, B outside 1..65535, n_views outside 1..63,
 * max_len outside 1..2^30.  Added without a version step: callers detect the addition by symbol. */
int aware_shift_views(const float* in, const int* in_off, const int* in_len, int B, const int* d, int n_views, float* out,
                      const int* out_off, int max_len, void* stream);

/* ---- scanning long recordings (EXTENSION, parity unpinned: the reference reads one payload per clip)----------------------
 * A file in which only a part is marked reads nothing as a whole.  The host detects every file in windows, window w at the
 * n_sync views of the offset search (aware_detect on rows with overlapping in_offsets, window-major, file after file), and
 * these two entries, one launch each on `stream`, read one payload per marked span.  win_off is a HOST int [B + 1]: file b owns
 * the windows win_off[b] .. win_off[b + 1] - 1 of W = win_off[B]; it starts at 0 and never falls.
 * aware_scan_select, one wave per window:
 *   values [W][n_sync][L] f32;  c_j = mean_l |values[w][j][l] - centre| in aware_sync_select's order,
 *   j* = the smallest j with the largest c_j (a NaN c_j never wins; all NaN: j* = 0 and c = -1);
 *   win_conf[w] = c_j*, win_view[w] = j*, win_values[w][0 : L] = values[w][j*],
 *   bit l % 32 of win_bits[w][l / 32] = values[w][j*][l] > centre  (uint32 [W][ceil(L / 32)], the unused bits zero).
 * aware_scan_segments, one workgroup per file; win_off_dev is the same B + 1 offsets on the device:
 *   window w is marked where win_conf[w] >= min_confidence (a NaN is never marked); a marked w continues the run of w - 1
 *   where that is marked too and their bits differ in at most max_flip places, and opens a new run otherwise.
 *   n_seg[b] = the runs of file b.  For its first max_segments runs r, at [b][r] of the seg_* arrays ([B][max_segments]):
 *   seg_first, seg_last = the run's first and last window, counted from the file's first; seg_peak = the smallest w of the
 *   run with the largest win_conf, counted likewise; seg_view = win_view[peak]; seg_conf = win_conf[peak];
 *   seg_values[b][r][l] = centre + (sum_w win_conf[w] (win_values[w][l] - centre)) / (sum_w win_conf[w]), both sums in f32
 *   over the run's windows in ascending order, every operation rounded on its own.  Slots beyond a file's runs are not
 *   written.
 * AWARE_E_BADARG, before anything is launched: a null pointer, values == win_values, B < 1, n_sync outside 1..64, L outside
 * 1..512, a centre or min_confidence that is not finite, max_flip < 0, max_segments < 1, a win_off that does not start at 0,
 * falls, or holds no window.  Added without a version step: callers detect the addition by symbol. */
int aware_scan_select(const float* values, const int* win_off, int B, int n_sync, int L, float centre, float* win_conf,
                      int* win_view, float* win_values, uint32_t* win_bits, void* stream);
int aware_scan_segments(const float* win_conf, const int* win_view, const float* win_values, const uint32_t* win_bits,
                        const int* win_off, const int* win_off_dev, int B, int L, float centre, float min_confidence,
                        int max_flip, int max_segments, int* n_seg, int* seg_first, int* seg_last, int* seg_peak,
                        int* seg_view, float* seg_conf, float* seg_values, void* stream);

/* ---- coded payloads: the Viterbi decoder (EXTENSION, no counterpart in the reference) -------------------------------------
 * A payload may be a frame of a zero-terminated convolutional code of constraint length 7 with a CRC (the definition is
 * aware_amd/utils/watermark/fec.py): rate_n = 2 has the generators (0171, 0133), rate_n = 3 has
 * (0133, 0171, 0165).  This entry decodes R rows of detector outputs in one launch on `stream`, one wave per row:
 *   values [R][L] f32;  y_i = values[r][i] - centre, 0 where that is not finite;  T = L / rate_n steps, the last
 *   L - rate_n T values ignored;  k = T - 6 - crc_bits message bits.  Path metrics in f32 from 0 for state 0 and -inf
 *   elsewhere; the metric of the branch from s_x = ((d & 31) << 1) | x into d is ((pm[s_x] + o_0 y_nt) + o_1 y_nt+1) + o_2 y_nt+2
 *   with o_g = +-1 the branch's output bit, every addition rounded on its own; x = 1 exactly where m_1 > m_0.
 *   bits [R][ceil(T / 32)] u32: bit t % 32 of word t / 32 is the decoded input bit of step t (message, CRC MSB first, 6 tail
 *   bits), traced back from state 0, the unused bits zero;  metric[r] = pm[0] after the last step;
 *   valid[r] = 1 where the metric is finite and (crc_bits > 0) the decoded CRC equals the CRC of the decoded message (bitwise,
 *   MSB first, register all ones at the start, no final xor; polynomial 0x07 or 0x1021), else 0;
 *   corrected[r] = the positions i < rate_n T where (y_i > 0) differs from the re-encoded decoded sequence.
 * AWARE_E_BADARG, before anything is launched: a null pointer, R outside 1..2^20, L outside 1..512, rate_n not 2 or 3,
 * crc_bits not 0, 8 or 16, a centre that is not finite, L / rate_n - 6 - crc_bits < 1.  Added without a version step:
 * callers detect the addition by symbol. */
int aware_viterbi_decode(const float* values, int R, int L, float centre, int rate_n, int crc_bits, uint32_t* bits,
                         float* metric, int* valid, int* corrected, void* stream);

/* ---- bare GEMM (tests / roofline): C[M][N] = A[M][K] * Bt[N][K]^T + bias ------------------------------ */
int aware_gemm_nt(const float* A, int lda, const float* Bt, int ldb, const float* bias, float* C, int ldc,
                  int M, int N, int K, void* stream);
/* same with an explicit tile configuration: variant 0 = automatic, 1..16 = fixed (tuning aid; all
 * configurations produce bit-identical results) */
int aware_gemm_nt_variant(const float* A, int lda, const float* Bt, int ldb, const float* bias, float* C, int ldc,
                          int M, int N, int K, int variant, void* stream);

/* ---- the clip-aligned conv block alone (tests / roofline) ----------------------------------------------
 * One Conv1dBlock of the detector (detection/modules/conv1d.py:38-42) on a uniform batch: clip b owns rows
 * [b*32*ceil(Tp/32), +Tp) of A and C (the rest of each 32-row group is padding, written as zero).
 *   epi 0: C = A*Bt^T + bias          epi 1: C = LeakyReLU_0.2(InstanceNorm_t(A*Bt^T + bias)), rstd_io[b][n] written
 *   epi 2: A is dL/d(output of the previous block), act that output; C = dL/d(its pre-norm conv output)
 * mode 0 runs the f32-MFMA kernel on Bt [N][K]; mode 1 the bf16 matrix-pipe kernel on Bpk, the same matrix split
 * exactly into three bf16 planes and re-ordered by aware_x3_pack (host buffers; aware_x3_packed_bytes bytes);
 * six partial products per multiply-add, f32 accumulation: f32-equivalent results (N % 128 == 0, K % 64 == 0). */
size_t aware_x3_packed_bytes(int N, int K);
int aware_x3_pack(const float* host_wt, int N, int K, void* host_out);
int aware_gemm_clip(const float* A, int lda, const float* Bt, int ldb, const void* Bpk, const float* bias, float* C,
                    int ldc, int B, int Tp, int N, int K, int epi, float* rstd_io, const float* act, int mode,
                    void* stream);
/* The same forward block (epi 1, bf16 matrix-pipe kernel) as the embed loop runs it for the block in front of the skinny last
 * conv (detection/multibit_detector_net.py:58-70: 1024 -> 40): besides C and rstd_out the epilogue writes the split-K
 * partials of the NEXT conv, zpart [N/128][B*32*ceil(Tp/32)][CL] with  sum_s zpart[s] = C * Wlast^T  (no bias).
 * lastpk: dev, aware_x3_pack of Wlast [16*ceil(CL/16)][N] (rows beyond CL zero).  2 <= CL <= 48.  Test / roofline entry. */
int aware_gemm_clip_last(const float* A, int lda, const void* Bpk, const float* bias, float* C, int ldc, int B, int Tp,
                         int N, int K, float* rstd_out, const void* lastpk, float* zpart, int CL, void* stream);
/* The same block on the DEFAULT conv pipe of the embed loop (csrc/gemm_h2.hip): the f16 matrix pipe with every f32 operand
 * written as two binary16 terms after a power-of-two scaling (per output channel for the weights, per clip for A), three
 * partial products per multiply-add, f32 accumulation; representation error <= 2^-23 relative per operand (one f32 ulp; rms 2^-24.5), the l_a l_b term (<= 2^-22) dropped.
 * Bt: DEV [N][K] (row pitch ldb); the entry packs it and computes the clips' max |A| into `workspace`
 * (>= aware_gemm_clip_h2_workspace_bytes).  epi 0..2 as aware_gemm_clip; lastpk / zpart / CL: as aware_gemm_clip_last (epi 1,
 * may be NULL / 0); amax_out: dev [B][64] partial maxima of |C| per clip (N/16 written per clip) or NULL.
 * N % 128 == 0, K % 64 == 0, K <= 1024. */
size_t aware_gemm_clip_h2_workspace_bytes(int B, int N, int K);
int aware_gemm_clip_h2(const float* A, int lda, const float* Bt, int ldb, const float* bias, float* C, int ldc, int B, int Tp,
                       int N, int K, int epi, float* rstd_io, const float* act, const void* lastpk, float* zpart, int CL,
                       float* amax_out, void* workspace, size_t workspace_bytes, void* stream);
/* The same with the form of the kernel chosen by the caller, so that a test can hold the two forms against each other on one
 * set of operands: tile 0 or 1 = 8 waves x 16 columns per workgroup (128-column slabs; what aware_gemm_clip_h2 runs), 2 = the
 * wide form, 4 waves x 64 columns (256-column slabs).  The two forms give the same bits in C, rstd, amax_out and zpart.
 * tile 2 needs Tp <= 96 and N % 256 == 0, else AWARE_E_UNSUPPORTED. */
int aware_gemm_clip_h2_tile(const float* A, int lda, const float* Bt, int ldb, const float* bias, float* C, int ldc, int B,
                            int Tp, int N, int K, int epi, float* rstd_io, const float* act, const void* lastpk, float* zpart,
                            int CL, float* amax_out, void* workspace, size_t workspace_bytes, int tile, void* stream);
/* Which form aware_gemm_clip_h2_tile runs for these arguments (no launch): 1 = 128-column slabs, 2 = the wide form with the
 * accumulator-layout epilogue, 3 = the wide form with the row-major epilogue (16-byte loads and stores: ldc % 4 == 0, C and --
 * epi 2 -- act 16-byte aligned).  last != 0: epi 1 with lastpk / zpart.  Same bits in every form.  AWARE_E_* as that entry. */
int aware_gemm_clip_h2_form(const float* C, int ldc, const float* act, int Tp, int N, int K, int lda, int epi, int last, int tile);

#ifdef __cplusplus
}
#endif
#endif /* AWARE_HIP_H */
