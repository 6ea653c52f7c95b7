"""Object wrappers over the C ABI: plan, batch geometry, detector weights, embed session.

PyTorch-ROCm is used for device memory and streams only; every computation below is a
call into libaware_hip.so on `torch.cuda.current_stream()`.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Sequence

import numpy as np
import torch

from . import _lib
from ._lib import AwareHipError, DetectorArch, EmbedConfig, check, load_library, require_gpu

SPEC_STRIDE = 256         # floats per band row, narrow layout (a plan's own value: Plan.band_stride)
SPEC_STRIDE_WIDE = 576    # ... wide layout: a band outside bins 1..511 or wider than 256 bins
FULL_STRIDE = 520
CONV_PIPES = {"f16x2": 0, "f32": 1, "bf16x3": 2}
CONV_TILES = {"auto": 0, "narrow": 1, "wide": 2}       # aware_embed_config::conv_tile
LOSS_KINDS = {"push_extremes": 0, "mse": 1, "hinge": 2, "sign": 3, "push_sigmoid": 4, "ber": 5, "push_extremes_l1": 6,
              "bce": 8}


def band_stride(band_lo: int, band_hi: int) -> int:
    """Row layout of a card plan's band-limited arrays (band_stride_for, csrc/common.hpp): SPEC_STRIDE for a band inside bins
    1..511 at most 256 bins wide, SPEC_STRIDE_WIDE for any other band inside bins 0..512."""
    return SPEC_STRIDE if band_lo >= 1 and band_hi <= 511 and band_hi - band_lo + 1 <= SPEC_STRIDE else SPEC_STRIDE_WIDE


def general_band_stride(nband: int) -> int:
    """Row layout of a general plan's band-limited arrays (gen_plan_create, csrc/capi.hip): the band's bins rounded up to a
    multiple of 64 -- 2112 floats for all 2049 bins of n_fft 4096."""
    return (int(nband) + 63) // 64 * 64


def stored_channels(channels: Sequence[int]) -> list[int]:
    """Channel counts a detector stores for the caller's `channels` = [n_mels, hidden widths..., 2 * payload bits]
    (stored_channels, csrc/detector_image.hpp; tests/test_detector_image_host.py holds the two against each other): the mel
    bank and every hidden width as is when a multiple of 4, else rounded up to a multiple of 4 up to 64 and of 128 above; the
    last block rounded up to a multiple of 4 up to 64 and of 128 above.  The padding channels are zero and invisible in every
    result."""
    n = len(channels) - 1
    out = []
    for i, c in enumerate(channels):
        if i < n and c % 4 == 0:
            out.append(c)
        else:
            out.append((c + 3) // 4 * 4 if c <= 64 else (c + 127) // 128 * 128)
    return out


def training_refusal(channels: Sequence[int]) -> str | None:
    """Why the detector-training extension refuses a network of these channels (None: it serves them): it runs 128 mel bands,
    hidden widths that need no padding and at most 6 hidden blocks only (the C ABI returns AWARE_E_UNSUPPORTED)."""
    if channels[0] != 128:
        return f"n_mels = {channels[0]} (detector training supports 128 mel bands only)"
    if len(channels) - 1 > 7:
        return f"num_blocks = {len(channels) - 2} (detector training supports at most 6 blocks)"
    st = stored_channels(channels)
    if any(a != b for a, b in zip(channels[1:-1], st[1:-1])):
        return f"n_filters = {list(channels[1:-1])} (detector training supports hidden widths that are multiples of 4 only)"
    return None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


GENERAL_NFFT = (256, 512, 1024, 2048, 4096)
PLAN_GENERAL = 1          # aware_plan_create_ex flag: the general kernels even for the card geometry, and the loop on them
WINDOWS = {"hann": 0, "hamming": 1}


def check_geometry(n_fft: int, hop: int, win_length: int, window: str = "hann"):
    """The STFT geometries the library serves (no GPU needed): NotImplementedError for an n_fft outside
    GENERAL_NFFT, ValueError for a hop / win_length outside 1..n_fft or an unknown window."""
    if window not in WINDOWS:
        raise ValueError(f"Invalid window type: {window}")       # utils/audio/stft.py:25
    if int(n_fft) not in GENERAL_NFFT:
        raise NotImplementedError(f"n_fft = {n_fft} is not supported: the HIP STFT kernels serve n_fft in {GENERAL_NFFT}")
    if not 1 <= int(hop) <= int(n_fft):
        raise ValueError(f"hop_length must lie in 1..n_fft = {n_fft}, got {hop}")
    if not 1 <= int(win_length) <= int(n_fft):
        raise ValueError(f"win_length must lie in 1..n_fft = {n_fft}, got {win_length}")


def nola_ok(n_fft: int, hop: int, win_length: int, window: str, n_samples: int) -> bool:
    """torch.istft's NOLA condition for a clip of n_samples samples (host-side, aware_nola_check): False where torch.istft
    raises because the window's overlap-add envelope drops below 1e-11 inside the trimmed output."""
    check_geometry(n_fft, hop, win_length, window)
    rc = load_library().aware_nola_check(int(n_fft), int(hop), int(win_length), WINDOWS[window], int(n_samples))
    if rc not in (0, -1):
        check(rc, "aware_nola_check")
    return rc == 0


CARD_GEOMETRY = (1024, 256, 1024)


def require_card_geometry(who: str, n_fft: int, hop: int, win_length: int, general_geometry: bool = False,
                          window: str = "hann"):
    """Without the key `general_geometry` the embed / detect loop runs on the model card's STFT geometry only.  With it the
    loop takes the general route at every geometry check_geometry accepts, the card's included."""
    if general_geometry:
        check_geometry(n_fft, hop, win_length, window)
        return
    if (int(n_fft), int(hop), int(win_length)) != CARD_GEOMETRY:
        raise NotImplementedError(f"{who}: frame_length / hop_length / win_length {n_fft} / {hop} / {win_length} is not "
                                  f"supported; the embed and detect kernels run on the model card's geometry "
                                  f"{CARD_GEOMETRY[0]} / {CARD_GEOMETRY[1]} / {CARD_GEOMETRY[2]} only unless the key "
                                  f"general_geometry is set (general_geometry=True, or `general_geometry: true` in the card)")


def refuse_general_geometry(feature: str, hint: str = ""):
    """What the general route does not serve: its kernels or its offsets are built on the card geometry (hop 256, a
    512-sample pooling period).  NotImplementedError naming the feature and the key; `hint` follows the message."""
    raise NotImplementedError(f"{feature} is not supported with general_geometry=True: it runs on the model card's STFT "
                              f"geometry {CARD_GEOMETRY[0]} / {CARD_GEOMETRY[1]} / {CARD_GEOMETRY[2]} only (key general_geometry off)"
                              + hint)


# the chain kinds the general route serves (aware_embed_set_general_chain): those that do not split a chain
GENERAL_CHAIN_KINDS = ("gaussian_noise", "sample_suppression", "gain_envelope")


def check_general_chain(chain):
    """A parsed chain for the general route (keys general_geometry and general_loop_attacks): NotImplementedError naming the
    first entry of a kind its kernels do not serve."""
    for j, a in enumerate(chain):
        if a["kind"] not in GENERAL_CHAIN_KINDS:
            raise NotImplementedError(f"loop_attacks[{j}] ({a['kind']}) is not supported with general_geometry=True: the general "
                                      f"route serves the kinds {', '.join(GENERAL_CHAIN_KINDS)} (key general_loop_attacks); "
                                      f"every other kind runs on the model card's STFT geometry only")


def check_general_clips(who: str, n_fft: int, hop: int, win_length: int, window: str, lengths, embed: bool = True):
    """The clips a general plan takes, checked on the host before any launch; ValueError naming the clip.  Every clip needs
    more than n_fft/2 samples (torch.stft's reflect padding).  For embedding it also has to pass torch.istft's NOLA
    condition (nola_ok) and leave a synthesis (hop * (T - 1) samples, T = 1 + n // hop frames) that the loop's second STFT
    can pad: more than n_fft/2 samples, or so few frames (T < 4, one pooled frame) that every block's InstanceNorm reads 0
    whatever the spectrum holds."""
    for i, n in enumerate(int(x) for x in lengths):
        if n <= n_fft // 2:
            raise ValueError(f"{who}: clip {i} has {n} samples; every clip needs more than n_fft/2 = {n_fft // 2}")
        if not embed:
            continue
        if not nola_ok(n_fft, hop, win_length, window, n):
            raise ValueError(f"{who}: clip {i} ({n} samples) fails the NOLA condition of torch.istft for n_fft {n_fft}, hop "
                             f"{hop}, win_length {win_length}, {window} window (the window's overlap-add envelope drops below "
                             f"1e-11 inside the output)")
        frames = 1 + n // hop
        if frames < 2 or (hop * (frames - 1) <= n_fft // 2 and frames >= 4):
            raise ValueError(f"{who}: clip {i} ({n} samples) synthesises to {hop * (frames - 1)} samples at hop {hop}; the loop's "
                             f"second STFT needs more than n_fft/2 = {n_fft // 2}")


def refuse_initial_pool(feature: str, pool):
    """What a detector with an initial pool other than (2, 2) does not serve: the searches, whose offsets and minimum lengths
    are built on the 512-sample period of the (2, 2) pool (hop 256 times the pool's stride).  NotImplementedError naming the
    feature and the pool."""
    raise NotImplementedError(f"{feature} is not supported with the initial pool (size {pool[0]}, stride {pool[1]}): its "
                              f"offsets assume the 512-sample read-out period of the (2, 2) pool, and this detector's is "
                              f"{256 * pool[1]} samples")


def conv_rows(rows: int, blocks: int, kernel_size: int, stride: int, padding: int) -> int:
    """Rows left of `rows` pooled rows behind `blocks` blocks of a detector of temporal convolutions: L -> floor((L + 2 p -
    k) / s) + 1 per block, 0 once a block has no output row (torch's conv1d raises there).  Mirror of conv_rows in
    csrc/conv_taps.hpp (aware_conv_rows)."""
    for _ in range(blocks):
        a = rows + 2 * padding - kernel_size
        rows = 0 if a < 0 else a // stride + 1
    return rows


def pool_rows(frames: int, size: int, stride: int) -> int:
    """Rows a clip of `frames` STFT frames enters block 0 with, behind the detector's initial pool AvgPool1d(size, stride):
    floor((frames - size) / stride) + 1, and 0 for frames < size (torch's avg_pool1d raises there).  pool_rows(T, 2, 2) ==
    T // 2.  Mirror of pool_rows in csrc/conv_taps.hpp (aware_pool_rows)."""
    return 0 if frames < size else (frames - size) // stride + 1


def check_tap_clips(who: str, frames, blocks: int, conv, pool=(2, 2)):
    """The clips a detector of `blocks` blocks with conv = (kernel_size, stride, padding) behind the initial pool = (size,
    stride) takes, checked on the host before any launch: ValueError naming the first clip (of `frames` STFT frames each) that
    the pool or some block leaves without a row.  The C ABI returns AWARE_E_BADARG for such a batch.  1x1 convolutions after
    the (2, 2) pool take every clip."""
    k, s, p = conv
    pool = tuple(pool)
    if (k, s, p) == (1, 1, 0) and pool == (2, 2):
        return
    for i, t in enumerate(int(x) for x in frames):
        rows = [conv_rows(pool_rows(t, *pool), j, k, s, p) for j in range(blocks + 1)]
        if rows[0] < 1:
            raise ValueError(f"{who}: clip {i} has {t} frames, and the initial pool of the detector (size {pool[0]}, stride "
                             f"{pool[1]}) leaves 0 rows of them: it needs at least {pool[0]} frames")
        if rows[-1] < 1:
            blk = next(j for j in range(1, blocks + 1) if rows[j] < 1)
            raise ValueError(f"{who}: clip {i} has {rows[0]} pooled rows ({t} frames), and block {blk - 1} of the detector "
                             f"(kernel_size {k}, stride {s}, padding {p}) leaves 0 rows of its {rows[blk - 1]}; rows per "
                             f"block: {rows[:blk + 1]}")


class Plan:
    """FFT tables + window + embedding band (aware_plan).  The card geometry (1024 / 256 / 1024) gives the card plan of the
    embed / detect loop; any other supported geometry (or general=True) a general plan: stft / istft / stft_bwd / istft_bwd
    on spectra of `spectrum_stride` complex values per row, and with general=True (the flag PLAN_GENERAL, what the key
    general_geometry passes) also the loop's general route, on band rows of `band_stride` floats (the band's bins rounded up
    to a multiple of 64), when the band lies inside bins 0..n_fft/2."""

    def __init__(self, n_fft=1024, hop=256, win_length=1024, window="hann", band_bins=(32, 256), general=False):
        require_gpu()
        self.lib = load_library()
        wid = WINDOWS.get(window)
        if wid is None:
            raise ValueError(f"Invalid window type: {window}")       # utils/audio/stft.py:25
        h = C.c_void_p()
        rc = self.lib.aware_plan_create_ex(C.byref(h), n_fft, hop, win_length, wid, int(band_bins[0]), int(band_bins[1]),
                                           PLAN_GENERAL if general else 0)
        if rc == -2 and int(n_fft) not in GENERAL_NFFT:
            raise NotImplementedError(f"n_fft = {n_fft} is not supported: the HIP STFT kernels serve n_fft in {GENERAL_NFFT}")
        check(rc, "aware_plan_create")
        self.h = h
        self.n_fft, self.hop, self.band_bins = n_fft, hop, (int(band_bins[0]), int(band_bins[1]))
        self.win_length, self.window = win_length, window
        self.nband = self.band_bins[1] - self.band_bins[0] + 1
        self.spectrum_stride = self.lib.aware_plan_spectrum_stride(h)
        self.band_stride = self.lib.aware_plan_band_stride(h)      # floats per row of the band-limited arrays
        self.general = bool(self.lib.aware_plan_is_general(h))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.aware_plan_destroy(self.h)
                self.h = None
        except Exception:
            pass


class Batch:
    """Ragged batch geometry (aware_batch)."""

    def __init__(self, lengths: Sequence[int], in_offsets: Sequence[int] | None = None, plan: Plan | None = None):
        """plan: build the geometry for that plan (frames by its hop, length rule by its n_fft: the batch a general plan
        needs); None: the card geometry."""
        require_gpu()
        self.lib = load_library()
        self.lengths = [int(x) for x in lengths]
        self.B = len(self.lengths)
        arr = (C.c_int * self.B)(*self.lengths)
        if in_offsets is None:
            self.in_offsets = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64).tolist()
            off = None
        else:
            self.in_offsets = [int(x) for x in in_offsets]
            off = (C.c_int * self.B)(*self.in_offsets)
        h = C.c_void_p()
        if plan is None:
            rc = self.lib.aware_batch_create(C.byref(h), self.B, arr, off)
        else:
            rc = self.lib.aware_batch_create_for_plan(C.byref(h), plan.h, self.B, arr, off)
        self.plan = plan
        if rc == -1:
            half = 512 if plan is None else plan.n_fft // 2
            raise ValueError(f"every clip needs more than n_fft/2 = {half} samples")
        check(rc, "aware_batch_create")
        self.h = h
        self.total_frames = self.lib.aware_batch_total_frames(h)
        self.total_pooled = self.lib.aware_batch_total_pooled(h)
        self.total_out = self.lib.aware_batch_total_out(h)
        self.frames = [self.lib.aware_batch_frames(h, i) for i in range(self.B)]
        self.out_offsets = [self.lib.aware_batch_out_offset(h, i) for i in range(self.B)]
        self.out_lengths = [self.lib.aware_batch_out_length(h, i) for i in range(self.B)]
        self.frame_offsets = np.concatenate([[0], np.cumsum(self.frames)]).tolist()
        self.total_in = self.in_offsets[-1] + self.lengths[-1]
        self.scratch_bytes = self.lib.aware_batch_scratch_bytes(h)
        # the run lengths the library chose for this batch (read-only): hop blocks per synthesis / loop-attack segment, frames
        # per analysis run
        self.synth_run = self.lib.aware_batch_synth_run(h)
        self.analysis_run = self.lib.aware_batch_analysis_run(h)
        self.uniform = len(set(self.lengths)) == 1 and in_offsets is None

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.aware_batch_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def scratch(self):
        return torch.empty(self.scratch_bytes, dtype=torch.uint8, device=_dev())

    # ---- ragged <-> list helpers (plumbing) ----
    def pack(self, clips) -> torch.Tensor:
        """list of 1-D float arrays/tensors -> one device tensor laid out at in_offsets."""
        out = torch.zeros(self.total_in, dtype=torch.float32, device=_dev())
        for c, o, n in zip(clips, self.in_offsets, self.lengths):
            out[o:o + n] = torch.as_tensor(c, dtype=torch.float32)
        return out

    def unpack_out(self, flat: torch.Tensor):
        return [flat[o:o + n] for o, n in zip(self.out_offsets, self.out_lengths)]


def stft(plan: Plan, batch: Batch, audio: torch.Tensor, normalize=False) -> torch.Tensor:
    """Full one-sided spectrum, frame-major [total_frames, plan.spectrum_stride] complex64 (bins 0..n_fft/2 valid; 520 and
    0..512 for the card plan)."""
    spec = torch.empty((batch.total_frames, plan.spectrum_stride), dtype=torch.complex64, device=audio.device)
    scr = batch.scratch()
    check(plan.lib.aware_stft(plan.h, batch.h, _ptr(audio), int(normalize), _ptr(spec), _ptr(scr), _stream()), "aware_stft")
    return spec


def istft(plan: Plan, batch: Batch, spec: torch.Tensor, normalize=False) -> torch.Tensor:
    out = torch.empty(batch.total_out, dtype=torch.float32, device=spec.device)
    scr = batch.scratch()
    rc = plan.lib.aware_istft(plan.h, batch.h, _ptr(spec), int(normalize), _ptr(out), _ptr(scr), _stream())
    _check_nola(rc, plan, batch)
    check(rc, "aware_istft")
    return out


def _check_nola(rc: int, plan: Plan, batch: Batch):
    if rc == -1 and plan.general and batch.plan is plan:
        bad = [n for n in batch.lengths if not nola_ok(plan.n_fft, plan.hop, plan.win_length, plan.window, n)]
        if bad:
            raise RuntimeError(f"istft: window overlap-add envelope is below 1e-11 (NOLA condition violated) for n_fft "
                               f"{plan.n_fft}, hop {plan.hop}, win_length {plan.win_length}, {plan.window} window; torch.istft "
                               f"raises for this geometry too")


def stft_band(plan: Plan, batch: Batch, audio: torch.Tensor, normalize=True):
    mag = torch.empty((batch.total_frames, plan.band_stride), dtype=torch.float32, device=audio.device)
    ph = torch.empty((batch.total_frames, plan.band_stride), dtype=torch.complex64, device=audio.device)
    scr = batch.scratch()
    check(plan.lib.aware_stft_band(plan.h, batch.h, _ptr(audio), int(normalize), _ptr(mag), _ptr(ph), _ptr(scr), _stream()),
          "aware_stft_band")
    return mag, ph


def stft_bwd(plan: Plan, batch: Batch, grad_spec: torch.Tensor) -> torch.Tensor:
    """Backward of `stft` (normalize=False): grad_spec [total_frames, plan.spectrum_stride] complex64 -> grad_audio f32 laid
    out like the audio `stft` takes (clip b: lengths[b] samples at in_offsets[b]); any clip length > n_fft/2."""
    out = torch.zeros(batch.total_in, dtype=torch.float32, device=grad_spec.device)
    check(plan.lib.aware_stft_bwd(plan.h, batch.h, _ptr(grad_spec), _ptr(out), _stream()), "aware_stft_bwd")
    return out


def istft_bwd(plan: Plan, batch: Batch, grad_audio: torch.Tensor) -> torch.Tensor:
    """Backward of `istft` (normalize=False): grad_audio [total_out] -> grad_spec [total_frames, plan.spectrum_stride]
    complex64."""
    gs = torch.empty((batch.total_frames, plan.spectrum_stride), dtype=torch.complex64, device=grad_audio.device)
    rc = plan.lib.aware_istft_bwd(plan.h, batch.h, _ptr(grad_audio), _ptr(gs), _stream())
    _check_nola(rc, plan, batch)
    check(rc, "aware_istft_bwd")
    return gs


def polar_decompose(spec: torch.Tensor):
    lib = load_library()
    mag = torch.empty(spec.shape, dtype=torch.float32, device=spec.device)
    ph = torch.empty(spec.shape, dtype=torch.float32, device=spec.device)
    check(lib.aware_polar_decompose(_ptr(spec), _ptr(mag), _ptr(ph), spec.numel(), _stream()), "aware_polar_decompose")
    return mag, ph


def polar_decompose_bwd(spec, grad_mag, grad_phase):
    lib = load_library()
    gs = torch.empty_like(spec)
    check(lib.aware_polar_decompose_bwd(_ptr(spec), _ptr(grad_mag), _ptr(grad_phase), _ptr(gs), spec.numel(), _stream()),
          "aware_polar_decompose_bwd")
    return gs


def polar_assemble(mag: torch.Tensor, phase: torch.Tensor) -> torch.Tensor:
    lib = load_library()
    spec = torch.empty(mag.shape, dtype=torch.complex64, device=mag.device)
    check(lib.aware_polar_assemble(_ptr(mag), _ptr(phase), _ptr(spec), mag.numel(), _stream()), "aware_polar_assemble")
    return spec


def polar_assemble_bwd(mag, phase, grad_spec, need_mag=True, need_phase=True):
    lib = load_library()
    gm = torch.empty_like(mag) if need_mag else None
    gp = torch.empty_like(mag) if need_phase else None
    check(lib.aware_polar_assemble_bwd(_ptr(mag), _ptr(phase), _ptr(grad_spec), _ptr(gm), _ptr(gp), mag.numel(), _stream()),
          "aware_polar_assemble_bwd")
    return gm, gp


def waveform_normalize_bwd(x: "Ragged", grad_out: torch.Tensor) -> torch.Tensor:
    lib = load_library()
    gi = torch.empty_like(x.data)
    check(lib.aware_waveform_normalize_bwd(_ptr(x.data), _ptr(grad_out), _ptr(gi), _ptr(x.d_off), _ptr(x.d_len), x.B, _stream()),
          "aware_waveform_normalize_bwd")
    return gi


class OptClamp:
    """Any optimiser of the reference's registry (embedding/optimizers.py:3-20) as ONE kernel on the caller's tensors, followed by
    torch.clamp(param, lo, hi): the generic form of NAdamClamp for the plug-in seam (aware_opt_clamp_step).  `scheduler`: a
    table scheduler dict of embedding.schedulers.get_scheduler (or None)."""

    def __init__(self, param: torch.Tensor, name: str, num_steps: int, scheduler_name: str | None = None, scheduler_params=None,
                 **params):
        from .embedding.optimizers import get_optimizer, hyper_parameters, step_table
        from .embedding.schedulers import get_scheduler
        self.lib = load_library()
        self.param = param
        self.opt = get_optimizer(name, None, **params)
        sched = get_scheduler(scheduler_name, self.opt, num_steps, **(scheduler_params or {})) if scheduler_name else None
        if sched is not None and sched["plateau"] is not None:
            raise NotImplementedError("OptClamp: a firing ReduceLROnPlateau needs the per-clip state of an embed session")
        self.hyp = hyper_parameters(self.opt)          # before the table consumes the scheduler (CyclicLR cycles momentum / beta1)
        self.table = step_table(self.opt, num_steps, sched["torch"] if sched else None)
        self.s1 = torch.zeros_like(param)
        self.s2 = torch.zeros_like(param)
        self.t = 0

    def step(self, grad: torch.Tensor, lo: torch.Tensor | None = None, hi: torch.Tensor | None = None):
        from .embedding.optimizers import step_scalars
        self.t += 1
        c4, h8 = step_scalars(self.opt, self.table, self.t, hyp=self.hyp)
        check(self.lib.aware_opt_clamp_step(self.opt["kind"], _ptr(self.param), _ptr(grad), _ptr(self.s1), _ptr(self.s2), _ptr(lo),
                                            _ptr(hi), self.param.numel(), c4.ctypes.data_as(C.POINTER(C.c_float)),
                                            h8.ctypes.data_as(C.POINTER(C.c_float)), _stream()), "aware_opt_clamp_step")


class NAdamClamp:
    """torch.optim.NAdam (single tensor, defaults of cards/config.yaml) followed by torch.clamp(param, lo, hi), as ONE
    kernel on the caller's tensors (aware_nadam_clamp_step): the optimiser step of the reference's loop
    (embedding/multibit_embedder.py:112-117) for the plug-in seam."""

    def __init__(self, param: torch.Tensor, lr=0.1, betas=(0.9, 0.999), eps=1e-8, momentum_decay=4e-3):
        self.lib = load_library()
        self.param = param
        self.lr, self.betas, self.eps, self.md = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(momentum_decay)
        self.exp_avg = torch.zeros_like(param)
        self.exp_avg_sq = torch.zeros_like(param)
        self.mu_product = C.c_float(1.0)
        self.t = 0

    def step(self, grad: torch.Tensor, lo: torch.Tensor | None = None, hi: torch.Tensor | None = None):
        self.t += 1
        c3 = (C.c_float * 3)()
        check(self.lib.aware_nadam_coefficients(self.t, self.lr, self.betas[0], self.betas[1], self.md, C.byref(self.mu_product), c3),
              "aware_nadam_coefficients")
        check(self.lib.aware_nadam_clamp_step(_ptr(self.param), _ptr(grad), _ptr(self.exp_avg), _ptr(self.exp_avg_sq), _ptr(lo),
                                              _ptr(hi), self.param.numel(), c3, self.betas[0], self.betas[1], self.eps, _stream()),
              "aware_nadam_clamp_step")


def detector_backward(plan: Plan, det: "DetectorWeights", batch: Batch, mag: torch.Tensor, grad_values: torch.Tensor):
    """(values [B, n_bits], grad_mag [total_frames, plan.band_stride]) = forward and J^T grad_values of the frozen network."""
    det.check_clips("aware_detector_backward", batch)
    nbytes = plan.lib.aware_detector_backward_workspace_bytes(batch.h, det.h)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=mag.device)
    vals = torch.empty((batch.B, det.n_bits), dtype=torch.float32, device=mag.device)
    gmag = torch.empty((batch.total_frames, plan.band_stride), dtype=torch.float32, device=mag.device)
    gv = grad_values.contiguous().float()
    check(plan.lib.aware_detector_backward(det.h, batch.h, _ptr(mag), _ptr(gv), _ptr(vals), _ptr(gmag), _ptr(ws), nbytes, _stream()),
          "aware_detector_backward")
    return vals, gmag


def require_card_arch(det: "DetectorWeights", what: str):
    """The detector-training extension serves the model card's architecture on a band of the narrow layout, with the sizes of
    training_refusal, only (the C ABI returns AWARE_E_UNSUPPORTED)."""
    if not det.is_card:
        raise NotImplementedError(f"{what}: detector training supports the model card's architecture only "
                                  "(instance norm, leaky_relu blocks, tanh read-out)")
    if det.plan.band_stride != SPEC_STRIDE:
        raise NotImplementedError(f"{what}: detector training supports bands inside bins 1..511 at most 256 bins wide only; "
                                  f"the band {det.plan.band_bins} has the wide layout")
    why = training_refusal(det.channels)
    if why:
        raise NotImplementedError(f"{what}: {why}")


def detector_weight_gradients(plan: Plan, det: "DetectorWeights", batch: Batch, mag: torch.Tensor, grad_values: torch.Tensor):
    """EXTENSION (detector training): (values, grad_mag, [dL/dW_l], [dL/db_l]) of the network for the upstream gradient
    grad_values [B, n_bits] (aware_detector_weight_gradients)."""
    require_card_arch(det, "aware_detector_weight_gradients")
    lib = plan.lib
    nbytes = lib.aware_detector_train_workspace_bytes(batch.h, det.h)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=mag.device)
    vals = torch.empty((batch.B, det.n_bits), dtype=torch.float32, device=mag.device)
    gmag = torch.empty((batch.total_frames, plan.band_stride), dtype=torch.float32, device=mag.device)
    ch = det.channels
    gw = [torch.empty((ch[i + 1], ch[i]), dtype=torch.float32, device=mag.device) for i in range(len(ch) - 1)]
    gb = [torch.empty((ch[i + 1],), dtype=torch.float32, device=mag.device) for i in range(len(ch) - 1)]
    pw = (C.c_void_p * len(gw))(*[t.data_ptr() for t in gw])
    pb = (C.c_void_p * len(gb))(*[t.data_ptr() for t in gb])
    gv = grad_values.contiguous().float()
    check(lib.aware_detector_weight_gradients(det.h, batch.h, _ptr(mag), _ptr(gv), _ptr(vals), _ptr(gmag), pw, pb, _ptr(ws), nbytes,
                                              _stream()), "aware_detector_weight_gradients")
    return vals, gmag, gw, gb


def detector_train_gradients(plan: Plan, det: "DetectorWeights", batch: Batch, mag: torch.Tensor, target: torch.Tensor,
                             loss: str = "push_extremes", grad_weights=None, grad_biases=None):
    """EXTENSION (detector training): ONE forward + backward of the network with the loss evaluated on the device
    (aware_detector_train_gradients): (values [B, n_bits], per-clip losses [B], [dL/dW_l], [dL/db_l]) -- gradients of the SUM
    of the per-clip losses.  grad_weights / grad_biases: tensors to write into (e.g. views of one flat bucket)."""
    require_card_arch(det, "aware_detector_train_gradients")
    if loss == "bce":
        raise NotImplementedError("aware_detector_train_gradients: the loss bce needs a detector that ends in sigmoid, and "
                                  "detector training supports the model card's tanh read-out only")
    lib = plan.lib
    nbytes = lib.aware_detector_train_workspace_bytes(batch.h, det.h)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=mag.device)
    vals = torch.empty((batch.B, det.n_bits), dtype=torch.float32, device=mag.device)
    losses = torch.empty((batch.B,), dtype=torch.float32, device=mag.device)
    ch = det.channels
    gw = grad_weights or [torch.empty((ch[i + 1], ch[i]), dtype=torch.float32, device=mag.device) for i in range(len(ch) - 1)]
    gb = grad_biases or [torch.empty((ch[i + 1],), dtype=torch.float32, device=mag.device) for i in range(len(ch) - 1)]
    pw = (C.c_void_p * len(gw))(*[t.data_ptr() for t in gw])
    pb = (C.c_void_p * len(gb))(*[t.data_ptr() for t in gb])
    tg = target.contiguous().float()
    check(lib.aware_detector_train_gradients(det.h, batch.h, _ptr(mag), _ptr(tg), LOSS_KINDS[loss], _ptr(losses), _ptr(vals), None,
                                             pw, pb, _ptr(ws), nbytes, _stream()), "aware_detector_train_gradients")
    return vals, losses, gw, gb


def _host_arrays(arrays):
    """The float32 C-contiguous form of each of `arrays` and the C array of pointers to them, as the detector's entry points
    take weights, biases and BatchNorm maps (keep the first alive while the second is in use)."""
    keep = [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]
    return keep, (C.c_void_p * len(keep))(*[a.ctypes.data for a in keep])


class DetectorWeights:
    """Device copy of the frozen detector (aware_detector)."""

    def __init__(self, plan: Plan, mel_basis: np.ndarray, weights, biases, arch: dict = None, conv=None, pool=None):
        """arch: AWAREDetectorNet.architecture() (aware_detector_create_ex), or None for the model card's network.
        conv: (kernel_size, stride, padding) of a net of temporal convolutions, weights [cout, cin, kernel_size] per block
        (aware_detector_create_conv; needs arch), or None for 1x1 convolutions.
        pool: (initial_pool_size, initial_pool_stride) of a net with another initial pool (aware_detector_create_pool; needs
        arch), or None for the (2, 2) pool."""
        require_gpu()
        self.lib = load_library()
        self.plan = plan
        mel = self._mel = _host_arrays([mel_basis])[0][0]
        ws, wp = _host_arrays(weights)
        bs, bp = _host_arrays(biases)
        chans = [ws[0].shape[1]] + [w.shape[0] for w in ws]
        self.channels = chans
        self.n_bits = chans[-1] // 2
        nl = len(ws)
        self.conv = tuple(int(v) for v in conv) if conv is not None else (1, 1, 0)
        self.pool = tuple(int(v) for v in pool) if pool is not None else (2, 2)
        if conv is not None and arch is None:
            raise ValueError("DetectorWeights: conv needs arch (aware_detector_create_conv)")
        if pool is not None and arch is None:
            raise ValueError("DetectorWeights: pool needs arch (aware_detector_create_pool)")
        if any(w.ndim != (3 if conv is not None else 2) or (conv is not None and w.shape[2] != self.conv[0]) for w in ws):
            raise ValueError("DetectorWeights: weights are [cout, cin] per block, or [cout, cin, kernel_size] with conv")
        # the shortest entry point that takes the arguments given
        name, more = "aware_detector_create", []
        if arch is not None:
            a = DetectorArch(arch["activation"], arch["norm"], arch["final_activation"], None, None)
            if arch.get("scale") is not None:
                self._norm, a.norm_scale = _host_arrays(arch["scale"])
                shift, a.norm_shift = _host_arrays(arch["shift"])
                self._norm += shift
            name, more = "aware_detector_create_ex", [C.byref(a)]
            if pool is not None:
                name, more = "aware_detector_create_pool", more + [*self.conv, *self.pool]
            elif conv is not None:
                name, more = "aware_detector_create_conv", more + [*self.conv]
        h = C.c_void_p()
        check(getattr(self.lib, name)(C.byref(h), plan.h, C.c_void_p(mel.ctypes.data), mel.shape[0], nl, (C.c_int * (nl + 1))(*chans),
                                      wp, bp, *more), name)
        self.h = h
        self.is_card = bool(self.lib.aware_detector_is_card(h))

    def check_clips(self, who: str, batch: "Batch"):
        """check_tap_clips on the batch's clips, in front of every entry point that takes this detector."""
        check_tap_clips(who, batch.frames, len(self.channels) - 1, self.conv, self.pool)

    def update(self, weights, biases):
        """EXTENSION (detector training): replace the parameters in place (same shapes), aware_detector_update."""
        require_card_arch(self, "aware_detector_update")
        torch.cuda.synchronize()
        ws, wp = _host_arrays(weights)
        bs, bp = _host_arrays(biases)
        check(self.lib.aware_detector_update(self.h, C.c_void_p(self._mel.ctypes.data), wp, bp), "aware_detector_update")

    def update_device(self, weights, biases):
        """EXTENSION (detector training): the same from DEVICE tensors, asynchronous on the current stream -- no host round trip
        (aware_detector_update_device: copies, transposes and both packed images rebuilt by kernels)."""
        require_card_arch(self, "aware_detector_update_device")
        ws = [w if w.is_contiguous() else w.contiguous() for w in weights]
        bs = [b if b.is_contiguous() else b.contiguous() for b in biases]
        wp = (C.c_void_p * len(ws))(*[w.data_ptr() for w in ws])
        bp = (C.c_void_p * len(bs))(*[b.data_ptr() for b in bs])
        check(self.lib.aware_detector_update_device(self.h, wp, bp, _stream()), "aware_detector_update_device")

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.aware_detector_destroy(self.h)
                self.h = None
        except Exception:
            pass


def detect(plan: Plan, det: DetectorWeights, batch: Batch, audio: torch.Tensor) -> torch.Tensor:
    """AWAREDetector.detect for a ragged batch -> [B, n_bits] raw values (device)."""
    det.check_clips("aware_detect", batch)
    nbytes = plan.lib.aware_detect_workspace_bytes(batch.h, det.h)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=audio.device)
    out = torch.empty((batch.B, det.n_bits), dtype=torch.float32, device=audio.device)
    check(plan.lib.aware_detect(plan.h, det.h, batch.h, _ptr(audio), _ptr(out), _ptr(ws), nbytes, _stream()), "aware_detect")
    return out


def detector_forward(plan: Plan, det: DetectorWeights, batch: Batch, mag: torch.Tensor) -> torch.Tensor:
    det.check_clips("aware_detector_forward", batch)
    nbytes = plan.lib.aware_detect_workspace_bytes(batch.h, det.h)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=mag.device)
    out = torch.empty((batch.B, det.n_bits), dtype=torch.float32, device=mag.device)
    check(plan.lib.aware_detector_forward(det.h, batch.h, _ptr(mag), _ptr(out), _ptr(ws), nbytes, _stream()),
          "aware_detector_forward")
    return out


def mixture_struct(dev_mixture):
    """The C ABI's aware_loop_chain array of embedding.loop_attacks.device_mixture, and the entry arrays it points into
    (keep them alive as long as the array is used)."""
    keep = [(_lib.LoopAttackEx * len(ent))(*[_lib.LoopAttackEx(k, pr, (C.c_float * 4)(*p)) for k, pr, p in ent])
            for _, ent in dev_mixture]
    arr = (_lib.LoopChain * len(dev_mixture))(*[_lib.LoopChain(C.cast(a, C.POINTER(_lib.LoopAttackEx)), len(a), float(w))
                                                 for a, (w, _) in zip(keep, dev_mixture)])
    return arr, keep


def loop_mixture_draw(seeds, step: int, weights) -> torch.Tensor:
    """embedding.loop_attacks.mixture_choice on the device (aware_loop_mixture_draw): the chain each of the B seeds draws
    at `step` under `weights` (-1: none), int32 [B]."""
    lib = load_library()
    sd = torch.from_numpy(np.asarray([int(s) & 0xFFFFFFFF for s in seeds], dtype=np.uint32).view(np.int32)).to(_dev())
    out = torch.empty(len(seeds), dtype=torch.int32, device=_dev())
    w = (C.c_float * len(weights))(*[float(x) for x in weights])
    rc = lib.aware_loop_mixture_draw(_ptr(sd), len(seeds), int(step), w, len(weights), _ptr(out), _stream())
    if rc == -1:
        raise ValueError("loop_mixture_draw: refused (1..8 finite weights >= 0 with a sum <= 1, at least one seed)")
    check(rc, "aware_loop_mixture_draw")
    return out


class EmbedSession:
    """One batched run of AWAREEmbedder._optimize (aware_embed)."""

    def __init__(self, plan: Plan, det: DetectorWeights, batch: Batch, num_iterations=400, tolerance_db=6.0,
                 loss="push_extremes", lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8, momentum_decay=4e-3,
                 use_graph=True, conv_pipe="f16x2", fused_readout=True, dsp_path="stream", l1_weight=0.0, mel="taps",
                 conv_tile="auto"):
        """conv_pipe: "f16x2" (default: conv blocks of chip-filling uniform batches on the f16 matrix pipe, two-term operand
        split, three products -- gemm_h2.hip; everything else as "bf16x3"), "bf16x3" (bf16 matrix pipe, exact three-way operand
        split, six products -- gemm_x3.hip) or "f32" (f32-input MFMA);
        fused_readout=False selects the three-kernel read-out that ragged batches use; dsp_path: "stream" (default:
        streaming wave kernels) or "staged" (workgroup-staged kernels) for the STFT / iSTFT stages (aware_embed_config);
        conv_tile: the form of the f16 two-term conv kernel -- "auto" (default: chosen per launch by the session's plan), "narrow"
        (8 waves x 16 columns, 128-column slabs) or "wide" (4 waves x 64 columns, 256-column slabs, wherever it can run; the
        library refuses a session in which no launch can take it).  The forms give the same bits; conv_tiles() reports them."""
        self.lib = load_library()
        det.check_clips("aware_embed_create", batch)
        self.plan, self.det, self.batch = plan, det, batch
        if loss not in LOSS_KINDS:
            raise ValueError(f"Unknown loss type: {loss}. Available on the HIP path: {list(LOSS_KINDS)}")
        if conv_pipe not in CONV_PIPES:
            raise ValueError(f"Unknown conv_pipe: {conv_pipe}")
        if conv_tile not in CONV_TILES:
            raise ValueError(f"Unknown conv_tile: {conv_tile}")
        self.cfg = EmbedConfig(int(num_iterations), float(tolerance_db), LOSS_KINDS[loss], lr, beta1, beta2, eps,
                               momentum_decay, int(bool(use_graph)), CONV_PIPES[conv_pipe],
                               0 if fused_readout else 1, {"stream": 0, "staged": 1}[dsp_path], float(l1_weight),
                               {"taps": 0, "dense": 1}[mel], CONV_TILES[conv_tile])
        self.nbytes = self.lib.aware_embed_workspace_bytes(batch.h, det.h)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=_dev())
        h = C.c_void_p()
        check(self.lib.aware_embed_create(C.byref(h), plan.h, det.h, batch.h, C.byref(self.cfg), _ptr(self.ws),
                                          self.nbytes, _stream()), "aware_embed_create")
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.aware_embed_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def conv_tiles(self):
        """The form of each conv launch of this session (aware_embed_conv_tile): (forward, backward), one entry per conv block:
        2 = the wide form of the f16 two-term kernel, 1 = its 128-column form, 0 = another kernel / no such launch."""
        n = len(self.det.channels) - 1
        return ([int(self.lib.aware_embed_conv_tile(self.h, 0, l)) for l in range(n)],
                [int(self.lib.aware_embed_conv_tile(self.h, 1, l)) for l in range(n)])

    def set_optimizer(self, opt: dict, sched: dict):
        """Any optimiser / scheduler of the reference's registries (embedding.optimizers.get_optimizer /
        embedding.schedulers.get_scheduler dicts) instead of the model card's fused NAdam (aware_embed_set_optimizer)."""
        from .embedding.optimizers import hyper_parameters, step_table
        hyp, wd = hyper_parameters(opt)                # before the table consumes the scheduler (CyclicLR cycles momentum / beta1)
        tab = np.ascontiguousarray(step_table(opt, self.cfg.num_iterations, sched["torch"]), dtype=np.float64)
        oc = _lib.OptimizerConfig()
        oc.kind = opt["kind"]
        oc.hyp = (C.c_float * 8)(*hyp)
        oc.weight_decay = wd
        oc.table = tab.ctypes.data_as(C.POINTER(C.c_double))
        pl = sched["plateau"]
        oc.plateau = int(pl is not None)
        if pl:
            oc.patience, oc.factor, oc.threshold, oc.min_lr, oc.eps = pl["patience"], pl["factor"], pl["threshold"], pl["min_lr"], pl["eps"]
        oc.lr0 = float(tab[0, 3])
        check(self.lib.aware_embed_set_optimizer(self.h, C.byref(oc), _stream()), "aware_embed_set_optimizer")
        self._opt_table = tab

    def set_loop_attacks(self, chain, seeds, sample_rate: int = 16000):
        """Attack-aware embedding (EXTENSION; aware_embed_set_loop_attacks): a chain of embedding.loop_attacks entries
        applied to the normalised synthesis inside every iteration, drawn afresh per step from the per-clip `seeds`
        (B integers).  Before the first iterate(); an empty chain clears it.  The attacked signal of the last forward pass
        is `attacked`."""
        from .embedding import loop_attacks as la
        chain = la.parse_chain(chain)
        if not chain:
            check(self.lib.aware_embed_set_loop_attacks(self.h, None, 0, None, None, 0, _stream()), "aware_embed_set_loop_attacks")
            self.loop_attacks, self._la_ws = [], None
            return
        if len(seeds) != self.batch.B:
            raise ValueError(f"set_loop_attacks: {self.batch.B} clips but {len(seeds)} seeds")
        la.check_lengths(chain, sample_rate, self.batch.out_lengths)      # ValueError naming the clip, before any launch
        sd = (C.c_uint32 * self.batch.B)(*[int(s) & 0xFFFFFFFF for s in seeds])
        if any(a["kind"] not in ("gaussian_noise", "sample_suppression") for a in chain):
            # the entry points with four parameters per entry; chains of the two older kinds keep the older call
            ent = la.device_entries_ex(chain, sample_rate)
            arr = (_lib.LoopAttackEx * len(ent))(*[_lib.LoopAttackEx(k, pr, (C.c_float * 4)(*p)) for k, pr, p in ent])
            nbytes = self.lib.aware_embed_loop_attack_workspace_bytes_ex(self.batch.h, arr, len(ent))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=_dev())
            rc = self.lib.aware_embed_set_loop_attacks_ex(self.h, arr, len(ent), sd, _ptr(ws), nbytes, _stream())
        else:
            ent = la.device_entries(chain, sample_rate)
            arr = (_lib.LoopAttack * len(ent))(*[_lib.LoopAttack(k, p, pr) for k, p, pr in ent])
            nbytes = self.lib.aware_embed_loop_attack_workspace_bytes(self.batch.h, len(ent))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=_dev())
            rc = self.lib.aware_embed_set_loop_attacks(self.h, arr, len(ent), sd, _ptr(ws), nbytes, _stream())
        if rc == -1:
            raise ValueError("set_loop_attacks: refused (it has to precede the first iterate(); see aware_hip.h)")
        check(rc, "aware_embed_set_loop_attacks")
        self.loop_attacks, self._la_ws = chain, ws

    def set_general_chain(self, chain, seeds, sample_rate: int = 16000):
        """Attack-aware embedding on the general route (EXTENSION; aware_embed_set_general_chain): as
        set_loop_attacks for a session on a general plan, with the kinds of GENERAL_CHAIN_KINDS (NotImplementedError naming any
        other).  `seconds` and `period` become samples at `sample_rate`.  Before the first iterate(); an empty chain clears
        it, and the session launches what it launched before.  The attacked signal of the last forward pass is `attacked`."""
        from .embedding import loop_attacks as la
        chain = la.parse_chain(chain, sample_rate)
        if not chain:
            rc = self.lib.aware_embed_set_general_chain(self.h, None, 0, None, None, 0, _stream())
            if rc == -1:
                raise ValueError("set_general_chain: refused (it has to precede the first iterate(); see aware_hip.h)")
            check(rc, "aware_embed_set_general_chain")
            self.loop_attacks, self._la_ws = [], None
            return
        check_general_chain(chain)
        if len(seeds) != self.batch.B:
            raise ValueError(f"set_general_chain: {self.batch.B} clips but {len(seeds)} seeds")
        la.check_lengths(chain, sample_rate, self.batch.out_lengths)      # ValueError naming the clip, before any launch
        sd = (C.c_uint32 * self.batch.B)(*[int(s) & 0xFFFFFFFF for s in seeds])
        ent = la.device_entries_ex(chain, sample_rate)
        arr = (_lib.LoopAttackEx * len(ent))(*[_lib.LoopAttackEx(k, pr, (C.c_float * 4)(*p)) for k, pr, p in ent])
        nbytes = self.lib.aware_embed_general_chain_workspace_bytes(self.batch.h, arr, len(ent))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=_dev())
        rc = self.lib.aware_embed_set_general_chain(self.h, arr, len(ent), sd, _ptr(ws), nbytes, _stream())
        if rc == -1:
            raise ValueError("set_general_chain: refused (it has to precede the first iterate(); see aware_hip.h)")
        check(rc, "aware_embed_set_general_chain")
        self.loop_attacks, self._la_ws = chain, ws

    def set_loop_mixture(self, mixture, seeds, sample_rate: int = 16000):
        """Attack mixtures (EXTENSION; aware_embed_set_loop_mixture): a list of {"weight": w, "chain": [...]} of
        embedding.loop_attacks.parse_mixture; at every step each clip draws one chain (or none) from its seed and goes
        through it as under set_loop_attacks with that chain alone.  Before the first iterate(); an empty mixture clears
        it; a mixture and a chain replace each other.  The choices of the last forward pass are `choices`."""
        from .embedding import loop_attacks as la
        mixture = la.parse_mixture(mixture)
        if not mixture:
            rc = self.lib.aware_embed_set_loop_mixture(self.h, None, 0, None, None, 0, _stream())
            if rc == -1:
                raise ValueError("set_loop_mixture: refused (it has to precede the first iterate(); see aware_hip.h)")
            check(rc, "aware_embed_set_loop_mixture")
            self.loop_attacks, self.loop_mixture, self._la_ws = [], [], None
            return
        if len(seeds) != self.batch.B:
            raise ValueError(f"set_loop_mixture: {self.batch.B} clips but {len(seeds)} seeds")
        la.check_mixture_lengths(mixture, sample_rate, self.batch.out_lengths)     # ValueError naming chain and clip
        sd = (C.c_uint32 * self.batch.B)(*[int(s) & 0xFFFFFFFF for s in seeds])
        arr, keep = mixture_struct(la.device_mixture(mixture, sample_rate))
        nbytes = self.lib.aware_embed_loop_mixture_workspace_bytes(self.batch.h, arr, len(arr))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=_dev())
        rc = self.lib.aware_embed_set_loop_mixture(self.h, arr, len(arr), sd, _ptr(ws), nbytes, _stream())
        if rc == -1:
            raise ValueError("set_loop_mixture: refused (it has to precede the first iterate(); see aware_hip.h)")
        check(rc, "aware_embed_set_loop_mixture")
        self.loop_attacks, self.loop_mixture, self._la_ws = [], mixture, ws

    @property
    def choices(self):
        """The chain every clip drew in the last forward pass, int32 [B] (-1: none); None without a mixture."""
        p = self.lib.aware_embed_buffer(self.h, 14)
        if not p:
            return None
        off = p - self._la_ws.data_ptr()
        return self._la_ws[off: off + 4 * self.batch.B].view(torch.int32)

    @property
    def attacked(self):
        """The attacked signal z of the last forward pass (flat, clip b at batch.out_offsets[b]); None without a chain."""
        p = self.lib.aware_embed_buffer(self.h, 12)
        if not p:
            return None
        off = p - self._la_ws.data_ptr()
        return self._la_ws[off: off + 4 * self.batch.total_out].view(torch.float32)

    @property
    def impulse_responses(self):
        """The reverberation's impulse responses of the last forward pass, [B, 8192] (zero beyond the drawn length, the unit
        impulse where the entry did not fire); None unless the chain has a reverberation."""
        p = self.lib.aware_embed_buffer(self.h, 13)
        if not p:
            return None
        off = p - self._la_ws.data_ptr()
        return self._la_ws[off: off + 4 * 8192 * self.batch.B].view(torch.float32).view(self.batch.B, 8192)

    def begin(self, audio: torch.Tensor, target: torch.Tensor):
        self._audio, self._target = audio, target.contiguous().float()
        check(self.lib.aware_embed_begin(self.h, _ptr(audio), _ptr(self._target), _stream()), "aware_embed_begin")

    def iterate(self, n: int):
        rc = self.lib.aware_embed_iterate(self.h, int(n), _stream())
        if rc == -1:
            raise ValueError(f"iterate({n}): more than num_iterations = {self.cfg.num_iterations} steps since begin()")
        check(rc, "aware_embed_iterate")

    def gradient(self) -> torch.Tensor:
        g = torch.zeros((self.batch.total_frames, self.plan.band_stride), dtype=torch.float32, device=self.ws.device)
        check(self.lib.aware_embed_gradient(self.h, _ptr(g), _stream()), "aware_embed_gradient")
        return g

    def finish(self, rescale: torch.Tensor | None = None) -> torch.Tensor:
        out = torch.empty(self.batch.total_out, dtype=torch.float32, device=self.ws.device)
        check(self.lib.aware_embed_finish(self.h, _ptr(rescale), _ptr(out), _stream()), "aware_embed_finish")
        return out

    def _view(self, which, shape, dtype=torch.float32):
        p = self.lib.aware_embed_buffer(self.h, which)
        n = int(np.prod(shape))
        off = p - self.ws.data_ptr()
        itemsize = torch.empty((), dtype=dtype).element_size()
        return self.ws[off: off + n * itemsize].view(dtype).view(*shape)

    @property
    def loss(self):
        return self._view(0, (self.batch.B,))

    @property
    def best_loss(self):
        return self._view(1, (self.batch.B,))

    @property
    def pred(self):
        return self._view(2, (self.batch.B, self.det.n_bits))

    @property
    def coef(self):
        return self._view(3, (self.batch.total_frames, self.plan.band_stride))

    @property
    def best_coef(self):
        return self._view(4, (self.batch.total_frames, self.plan.band_stride))

    @property
    def bounds(self):
        return (self._view(5, (self.batch.total_frames, self.plan.band_stride)),
                self._view(6, (self.batch.total_frames, self.plan.band_stride)))

    @property
    def step(self):
        return self._view(8, (1,), torch.int32)

    def clip_learning_rates(self) -> np.ndarray:
        """Per-clip learning rates of a session whose optimiser was set with set_optimizer (device state, float64; they only
        differ from the table's rate under a firing ReduceLROnPlateau)."""
        if not self.lib.aware_embed_buffer(self.h, 11):
            raise AwareHipError("no optimiser was set with set_optimizer")
        return self._view(11, (self.batch.B,), torch.float64).cpu().numpy()


def gemm_nt(a: torch.Tensor, bt: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    lib = load_library()
    M, K = a.shape
    N = bt.shape[0]
    c = torch.empty((M, N), dtype=torch.float32, device=a.device)
    check(lib.aware_gemm_nt(_ptr(a), a.stride(0), _ptr(bt), bt.stride(0), _ptr(bias), _ptr(c), N, M, N, K, _stream()),
          "aware_gemm_nt")
    return c


def _pitched_f32(t: torch.Tensor, name: str, shape, dev):
    if tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or t.device != dev or t.stride(1) != 1 or t.stride(0) < shape[1]:
        raise ValueError(f"{name}: a {list(shape)} f32 view on a's device with unit column stride and a row pitch of at least "
                         f"{shape[1]}")


def gemm_nt_variant(a: torch.Tensor, bt: torch.Tensor, bias: torch.Tensor | None, variant: int, out=None) -> torch.Tensor:
    """C = a @ bt^T + bias on one tile configuration of the f32-MFMA GEMM (aware_gemm_nt_variant; tests / roofline).
    variant: 0 = the choice gemm_nt makes, 1..16 = the rows of gemm_dispatch (csrc/detector_kernels.hip); any other number is
    refused (AwareHipError "bad argument").  a: [M, K], bt: [N, K] and out: [M, N] may be row-pitched views (unit column
    stride, row pitch at least the row; the pitches of a and bt, like K, multiples of 4 as the ABI demands).  out=None
    allocates a contiguous [M, N].  Returns out."""
    lib = load_library()
    if a.dim() != 2 or bt.dim() != 2 or not a.is_cuda:
        raise ValueError("a: [M, K] and bt: [N, K] on the device")
    M, K = a.shape
    N = bt.shape[0]
    dev = a.device
    _pitched_f32(a, "a", (M, K), dev)
    _pitched_f32(bt, "bt", (N, K), dev)
    if bias is not None and (tuple(bias.shape) != (N,) or bias.dtype != torch.float32 or bias.device != dev
                             or not bias.is_contiguous()):
        raise ValueError("bias: a contiguous [N] f32 tensor on a's device")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=dev)
    else:
        _pitched_f32(out, "out", (M, N), dev)
    check(lib.aware_gemm_nt_variant(_ptr(a), a.stride(0), _ptr(bt), bt.stride(0), _ptr(bias), _ptr(out), out.stride(0), M, N, K,
                                    int(variant), _stream()), "aware_gemm_nt_variant")
    return out


def x3_pack(wt: torch.Tensor) -> torch.Tensor:
    """[N][K] f32 weights -> the three bf16 planes in MFMA fragment order (device uint8 tensor)."""
    lib = load_library()
    w = np.ascontiguousarray(wt.detach().cpu().numpy(), dtype=np.float32)
    N, K = w.shape
    nbytes = int(lib.aware_x3_packed_bytes(N, K))
    if nbytes == 0:
        raise AwareHipError("aware_x3_pack: N must be a positive multiple of 16")
    out = np.zeros(nbytes, dtype=np.uint8)
    check(lib.aware_x3_pack(w.ctypes.data, N, K, out.ctypes.data), "aware_x3_pack")
    return torch.from_numpy(out).cuda()


def gemm_clip(a: torch.Tensor, bt: torch.Tensor, bias, B: int, Tp: int, epi: int = 0, rstd=None, act=None,
              mode: int = 0, packed=None):
    """One clip-aligned conv block (tests / roofline).  a: [B*32*ceil(Tp/32), K]; bt: [N, K].
    Returns (C, rstd)."""
    lib = load_library()
    M, K = a.shape
    N = bt.shape[0]
    c = torch.empty((M, N), dtype=torch.float32, device=a.device)
    if rstd is None:
        rstd = torch.zeros((B, N), dtype=torch.float32, device=a.device)
    if mode == 1 and packed is None:
        packed = x3_pack(bt)
    check(lib.aware_gemm_clip(_ptr(a), a.stride(0), _ptr(bt), bt.stride(0), _ptr(packed), _ptr(bias), _ptr(c), N, B, Tp, N, K,
                              epi, _ptr(rstd), _ptr(act), mode, _stream()), "aware_gemm_clip")
    return c, rstd


def gemm_clip_h2(a: torch.Tensor, bt: torch.Tensor, bias, B: int, Tp: int, epi: int = 0, rstd=None, act=None, w_last=None,
                 tile: int = 0, out=None):
    """One clip-aligned conv block on the f16 two-term kernel (aware_gemm_clip_h2_tile; the embed loop's default conv pipe).
    tile: 0 or 1 = the 128-column form, 2 = the wide form (AwareHipError "unsupported" where it cannot run).
    out: the caller's C, an [M, N] view of any row pitch ldc = out.stride(0) >= N (act, where given, has the same pitch).
    Returns (C, rstd, amax_out[B, 64]) and, with w_last [CL, N] (epi 1), also zpart [N/128, M, CL]."""
    lib = load_library()
    M, K = a.shape
    N = bt.shape[0]
    dev = a.device
    btd = bt.to(dev).contiguous()
    if out is None:
        c = torch.empty((M, N), dtype=torch.float32, device=dev)
    else:
        c = out
        if tuple(c.shape) != (M, N) or c.stride(1) != 1 or c.stride(0) < N or c.dtype != torch.float32 or c.device != dev:
            raise ValueError("out: an [M, N] f32 view on a's device with unit column stride and a row pitch of at least N")
    ldc = c.stride(0)
    if act is not None and (act.stride(0) != ldc or act.stride(1) != 1):
        raise ValueError("act: the row pitch of C")
    if rstd is None:
        rstd = torch.zeros((B, N), dtype=torch.float32, device=dev)
    amax = torch.zeros((B, 64), dtype=torch.float32, device=dev)
    nbytes = int(lib.aware_gemm_clip_h2_workspace_bytes(B, N, K))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    pkl, zpart, CL = None, None, 0
    if w_last is not None:
        CL = w_last.shape[0]
        wl = torch.zeros((16 * ((CL + 15) // 16), N), dtype=torch.float32)
        wl[:CL] = w_last.detach().cpu().float()
        pkl = x3_pack(wl)
        zpart = torch.zeros((N // 128, M, CL), dtype=torch.float32, device=dev)
    check(lib.aware_gemm_clip_h2_tile(_ptr(a), a.stride(0), _ptr(btd), btd.stride(0), _ptr(bias), _ptr(c), ldc, B, Tp, N, K, epi,
                                      _ptr(rstd), _ptr(act), _ptr(pkl), _ptr(zpart), CL, _ptr(amax), _ptr(ws), nbytes, int(tile),
                                      _stream()), "aware_gemm_clip_h2_tile")
    torch.cuda.current_stream().synchronize()
    return (c, rstd, amax) if w_last is None else (c, rstd, amax, zpart)


def gemm_clip_h2_form(c: torch.Tensor, act, Tp: int, K: int, epi: int = 0, last: bool = False, tile: int = 0) -> int:
    """The form gemm_clip_h2 runs for this C (an [M, N] view, row pitch c.stride(0)) and act (aware_gemm_clip_h2_form):
    1 = 128-column, 2 = wide with the accumulator-layout epilogue, 3 = wide with the row-major epilogue."""
    lib = load_library()
    rc = int(lib.aware_gemm_clip_h2_form(_ptr(c), c.stride(0), _ptr(act), Tp, c.shape[1], K, K, epi, int(last), int(tile)))
    if rc < 0:
        check(rc, "aware_gemm_clip_h2_form")
    return rc


def gemm_clip_last(a: torch.Tensor, bt: torch.Tensor, bias, w_last: torch.Tensor, B: int, Tp: int):
    """The forward conv block + split-K partials of the next (skinny) conv, as the embed loop runs block 2
    (aware_gemm_clip_last).  a: [B*32*ceil(Tp/32), K]; bt: [N, K]; w_last: [CL, N].  Returns (C, rstd, zpart[N/128, M, CL])."""
    lib = load_library()
    M, K = a.shape
    N = bt.shape[0]
    CL = w_last.shape[0]
    clp = 16 * ((CL + 15) // 16)
    wl = torch.zeros((clp, N), dtype=torch.float32)
    wl[:CL] = w_last.detach().cpu().float()
    c = torch.empty((M, N), dtype=torch.float32, device=a.device)
    rstd = torch.zeros((B, N), dtype=torch.float32, device=a.device)
    zpart = torch.zeros((N // 128, M, CL), dtype=torch.float32, device=a.device)
    pk, pkl = x3_pack(bt), x3_pack(wl)                 # (named: both must stay allocated until the launch has been enqueued)
    check(lib.aware_gemm_clip_last(_ptr(a), a.stride(0), _ptr(pk), _ptr(bias), _ptr(c), N, B, Tp, N, K, _ptr(rstd),
                                   _ptr(pkl), _ptr(zpart), CL, _stream()), "aware_gemm_clip_last")
    torch.cuda.current_stream().synchronize()
    return c, rstd, zpart


# ---------------------------------------------------------------------------------------------
# ragged signal batches and the attack-stage entry points
# ---------------------------------------------------------------------------------------------
class Ragged:
    """B mono clips packed back to back in one device tensor (plumbing for the attack stage)."""

    def __init__(self, data: torch.Tensor, lengths: Sequence[int]):
        self.data = data
        self.lengths = [int(n) for n in lengths]
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64).tolist()
        self.B = len(self.lengths)
        self.max_len = max(self.lengths)
        dev = data.device
        self.d_off = torch.tensor(self.offsets, dtype=torch.int32, device=dev)
        self.d_len = torch.tensor(self.lengths, dtype=torch.int32, device=dev)

    @classmethod
    def from_list(cls, clips, dtype=torch.float32):
        lengths = [len(c) for c in clips]
        data = torch.cat([torch.as_tensor(np.asarray(c), dtype=dtype) for c in clips]).to(_dev())
        return cls(data, lengths)

    def select(self, indices):
        """sub-batch of the given clips (device-side gather of their spans)"""
        parts = [self.data[self.offsets[i]: self.offsets[i] + self.lengths[i]] for i in indices]
        return Ragged(torch.cat(parts) if len(parts) > 1 else parts[0].clone(), [self.lengths[i] for i in indices])

    def like(self, dtype=None):
        return Ragged(torch.empty_like(self.data, dtype=dtype or self.data.dtype), self.lengths)

    def to_list(self):
        flat = self.data.detach().cpu().numpy()
        return [flat[o:o + n] for o, n in zip(self.offsets, self.lengths)]

    def batch(self) -> Batch:
        return Batch(self.lengths)

    def _scratch(self):
        ps = (self.max_len + 4095) // 4096
        return torch.empty(self.B * (ps * 8 + 8) + 64, dtype=torch.uint8, device=self.data.device)


def waveform_normalize(x: Ragged) -> Ragged:
    lib = load_library()
    out = x.like()
    scr = x._scratch()
    check(lib.aware_waveform_normalize(_ptr(x.data), _ptr(out.data), _ptr(x.d_off), _ptr(x.d_len), x.B, x.max_len,
                                       _ptr(scr), _stream()), "aware_waveform_normalize")
    return out


def pcm_quantize(x: Ragged, bits: int) -> Ragged:
    lib = load_library()
    out = x.like()
    scr = x._scratch()
    rc = lib.aware_pcm_quantize(_ptr(x.data), _ptr(out.data), _ptr(x.d_off), _ptr(x.d_len), x.B, x.max_len, int(bits),
                                _ptr(scr), _stream())
    if rc == -1:
        raise ValueError(f"Unsupported PCM bit depth: {bits}")            # scripts/attacks.py:69
    check(rc, "aware_pcm_quantize")
    return out


def upfirdn(x: Ragged, h: torch.Tensor, up: int, down: int, half_len: int) -> Ragged:
    """polyphase resampler core; output length ceil(n*up/down) per clip (scipy.resample_poly)."""
    lib = load_library()
    out_len = [-(-n * up // down) for n in x.lengths]
    out = Ragged(torch.empty(sum(out_len), dtype=torch.float32, device=x.data.device), out_len)
    check(lib.aware_upfirdn(_ptr(x.data), _ptr(x.d_off), _ptr(x.d_len), _ptr(out.data), _ptr(out.d_off), _ptr(out.d_len),
                            x.B, out.max_len, _ptr(h), h.numel(), up, down, half_len, _stream()), "aware_upfirdn")
    return out


def iir(x: Ragged, b: np.ndarray, a: np.ndarray, zi: np.ndarray | None = None, filtfilt=False, out_f64=False) -> Ragged:
    """b, a: [B, ncoef] float64 (a[:,0] == 1) per clip; zi [B, ncoef-1] for filtfilt."""
    if min(x.lengths) < 1:                                  # aware_iir cannot see the device lengths: its precondition
        raise ValueError("iir: every clip needs at least one sample")
    lib = load_library()
    dev = x.data.device
    bd = torch.as_tensor(np.ascontiguousarray(b, dtype=np.float64), device=dev)
    ad = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
    ncoef = bd.shape[1]
    if filtfilt and min(x.lengths) <= 3 * ncoef:           # scipy.signal.filtfilt raises the same way (padlen = 3*max(len(a), len(b)))
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {3 * ncoef}.")
    zd = None if zi is None else torch.as_tensor(np.ascontiguousarray(zi, dtype=np.float64), device=dev)
    out = x.like(torch.float64 if out_f64 else torch.float32)
    scr = torch.empty(x.B * (x.max_len + 6 * ncoef), dtype=torch.float64, device=dev) if filtfilt else None
    check(lib.aware_iir(_ptr(x.data), _ptr(x.d_off), _ptr(x.d_len), x.B, x.max_len, _ptr(out.data), int(out_f64),
                        _ptr(bd), _ptr(ad), _ptr(zd), ncoef, int(filtfilt), _ptr(scr), _stream()), "aware_iir")
    return out


def decimate_interp(x: Ragged, factor: int) -> Ragged:
    """x[::factor] then np.interp back to the original length (float64 result), per clip."""
    lib = load_library()
    out = x.like(torch.float64)
    check(lib.aware_decimate_interp(_ptr(x.data), _ptr(x.d_off), _ptr(x.d_len), x.B, x.max_len, int(factor), _ptr(out.data),
                                    _stream()), "aware_decimate_interp")
    return out


def segment_cut(x: Ragged, starts: Sequence[int], cuts: Sequence[int], zero_fill: bool) -> Ragged:
    lib = load_library()
    dev = x.data.device
    out_len = x.lengths if zero_fill else [n - k for n, k in zip(x.lengths, cuts)]
    out = Ragged(torch.empty(sum(out_len), dtype=torch.float32, device=dev), out_len)
    st = torch.tensor(list(starts), dtype=torch.int32, device=dev)
    ct = torch.tensor(list(cuts), dtype=torch.int32, device=dev)
    check(lib.aware_segment_cut(_ptr(x.data), _ptr(x.d_off), _ptr(out.data), _ptr(out.d_off), _ptr(out.d_len), _ptr(st),
                                _ptr(ct), int(zero_fill), x.B, out.max_len, _stream()), "aware_segment_cut")
    return out


def gaussian_noise(x: Ragged, snr_db: float, seeds: Sequence[int]) -> Ragged:
    lib = load_library()
    dev = x.data.device
    out = x.like()
    sd = torch.tensor([int(s) & 0x7FFFFFFF for s in seeds], dtype=torch.int32, device=dev)
    scr = torch.empty(x.B * 8 + 64, dtype=torch.uint8, device=dev)
    check(lib.aware_gaussian_noise(_ptr(x.data), _ptr(out.data), _ptr(x.d_off), _ptr(x.d_len), x.B, x.max_len, _ptr(sd),
                                   float(snr_db), _ptr(scr), _stream()), "aware_gaussian_noise")
    return out


def reverb_ir(seeds: Sequence[int], step: int, entry: int, n_lo: int, n_hi: int, drr_db: float, stride: int = 8192):
    """The impulse responses embedding.loop_attacks.reverb_ir specifies, drawn on the device (aware_reverb_ir): (h [B, stride]
    float32, zero beyond the drawn length, and the lengths [B] int32) for the clips' seeds at optimiser step `step`, chain
    entry `entry`, lengths uniform on [n_lo, n_hi]."""
    lib = load_library()
    dev = _dev()
    sd = torch.from_numpy(np.array([int(s) & 0xFFFFFFFF for s in seeds], dtype=np.uint32).view(np.int32)).to(dev)
    h = torch.empty((len(seeds), int(stride)), dtype=torch.float32, device=dev)
    nh = torch.empty(len(seeds), dtype=torch.int32, device=dev)
    rc = lib.aware_reverb_ir(_ptr(sd), len(seeds), int(step), int(entry), int(n_lo), int(n_hi), float(drr_db), _ptr(h),
                             int(stride), _ptr(nh), _stream())
    if rc == -1:
        raise ValueError(f"reverb_ir: 2 <= n_lo <= n_hi <= min(8192, stride) and a finite drr_db are required; got "
                         f"{n_lo}, {n_hi}, stride {stride}, {drr_db}")
    check(rc, "aware_reverb_ir")
    return h, nh


def convolve(x: Ragged, h: torch.Tensor, nh: torch.Tensor, adjoint: bool = False) -> Ragged:
    """Per clip (h_b * x_b)[0 : n_b], causal and truncated, or with adjoint its transpose out[i] = sum_k h_b[k] x_b[i + k]
    (aware_convolve: partitioned FFT convolution).  h: device float32 [B, stride <= 8192], nh: device int32 [B] taps."""
    lib = load_library()
    if h.dim() != 2 or h.shape[0] != x.B or nh.numel() != x.B or not 1 <= h.shape[1] <= 8192:
        raise ValueError(f"convolve: h [B, <= 8192] and nh [B] are required for B = {x.B}; got {tuple(h.shape)}, {tuple(nh.shape)}")
    h = h.contiguous().float()
    nh = nh.contiguous().to(torch.int32)
    xin = x.data if x.data.dtype == torch.float32 else x.data.float()
    out = Ragged(torch.empty_like(xin), x.lengths)
    nbytes = lib.aware_convolve_workspace_bytes(x.B, x.max_len, sum(x.lengths), h.shape[1])
    ws = torch.empty(nbytes, dtype=torch.uint8, device=xin.device)
    check(lib.aware_convolve(_ptr(xin), _ptr(x.d_off), _ptr(x.d_len), x.B, x.max_len, _ptr(h), h.shape[1], _ptr(nh),
                             int(bool(adjoint)), _ptr(out.data), _ptr(ws), nbytes, _stream()), "aware_convolve")
    return out


def _resample_alone(who: str, entry: str, m_lo: int, m_hi: int, what: str, x: Ragged, m, adjoint: bool, out_lengths) -> Ragged:
    """What speed_change, stretch_ola and pitch_shift_ola share: the checks, the output and the call of the C entry `entry`."""
    lib = load_library()
    ms = [int(m)] * x.B if np.isscalar(m) else [int(v) for v in m]
    if len(ms) != x.B or any(v < m_lo or v > m_hi for v in ms):
        raise ValueError(f"{who}: {x.B} {what} are required; got {ms}")
    out_len = x.lengths if out_lengths is None else [int(n) for n in out_lengths]
    if len(out_len) != x.B or min(out_len) < 1:
        raise ValueError(f"{who}: {x.B} output lengths >= 1 are required; got {out_len}")
    xin = x.data if x.data.dtype == torch.float32 else x.data.float()
    out = Ragged(torch.empty(sum(out_len), dtype=torch.float32, device=xin.device), out_len)
    md = torch.tensor(ms, dtype=torch.int32, device=xin.device)
    # the C entry names the two sides of the forward operator: with adjoint, `out` is on the input side
    src, dst = (out, x) if adjoint else (x, out)
    check(getattr(lib, entry)(_ptr(xin), _ptr(src.d_off), _ptr(src.d_len), _ptr(out.data), _ptr(dst.d_off), _ptr(dst.d_len),
                              x.B, max(x.max_len, out.max_len), _ptr(md), int(bool(adjoint)), _stream()), entry)
    return out


def speed_change(x: Ragged, m, adjoint: bool = False, out_lengths=None) -> Ragged:
    """Per clip embedding.loop_attacks.speed_change at the speed offsets m (B integers, or one for all): clip b played at
    (65536 + m[b]) / 65536 of its speed (aware_speed_change), out_lengths[b] samples long (default: the clip's own length).
    With adjoint, x holds the gradient with respect to that output and the result, out_lengths long, is the gradient with
    respect to the input (out_lengths is then the forward pass's input lengths)."""
    return _resample_alone("speed_change", "aware_speed_change", -13520, 17034, "speed offsets within -13520..17034 (-+400 cents)",
                           x, m, adjoint, out_lengths)


def delete_samples(x: Ragged, start, k, adjoint: bool = False) -> Ragged:
    """Per clip embedding.loop_attacks.delete_samples (aware_delete_samples): the k[b] samples from start[b] on are cut out of
    clip b, the remainder moves up and zeros follow, so every clip keeps its length (B integers each, or one for all; k = 0
    is the identity).  With adjoint, x holds the gradient with respect to that output and the result is the gradient with
    respect to the input (zeros where the cut was)."""
    lib = load_library()
    st = [int(start)] * x.B if np.isscalar(start) else [int(v) for v in start]
    ks = [int(k)] * x.B if np.isscalar(k) else [int(v) for v in k]
    if len(st) != x.B or len(ks) != x.B or any(s < 0 or c < 0 or s + c > n for s, c, n in zip(st, ks, x.lengths)):
        raise ValueError(f"delete_samples: {x.B} cuts [start, start + k) inside the clips are required; got start = {st}, "
                         f"k = {ks} for lengths {list(x.lengths)}")
    xin = x.data if x.data.dtype == torch.float32 else x.data.float()
    out = Ragged(torch.empty(sum(x.lengths), dtype=torch.float32, device=xin.device), x.lengths)
    sd = torch.tensor(st, dtype=torch.int32, device=xin.device)
    kd = torch.tensor(ks, dtype=torch.int32, device=xin.device)
    check(lib.aware_delete_samples(_ptr(xin), _ptr(x.d_off), _ptr(x.d_len), x.B, x.max_len, _ptr(sd), _ptr(kd), _ptr(out.data),
                                   int(bool(adjoint)), _stream()), "aware_delete_samples")
    return out


def excerpt_tile(x: Ragged, start, length, adjoint: bool = False) -> Ragged:
    """Per clip embedding.loop_attacks.excerpt_tile (aware_excerpt_tile): the length[b] samples of clip b from start[b] on,
    repeated periodically until they fill the clip, so every clip keeps its length (B integers each, or one for all; a length
    equal to the clip's is the identity).  With adjoint, x holds the gradient with respect to that output and the result is the
    gradient with respect to the input: the sum over the periods in float32, zeros outside the excerpt."""
    lib = load_library()
    st = [int(start)] * x.B if np.isscalar(start) else [int(v) for v in start]
    ls = [int(length)] * x.B if np.isscalar(length) else [int(v) for v in length]
    if len(st) != x.B or len(ls) != x.B or any(s < 0 or c < 1 or s + c > n for s, c, n in zip(st, ls, x.lengths)):
        raise ValueError(f"excerpt_tile: {x.B} excerpts [start, start + length) inside the clips are required; got start = {st}, "
                         f"length = {ls} for lengths {list(x.lengths)}")
    xin = x.data if x.data.dtype == torch.float32 else x.data.float()
    out = Ragged(torch.empty(sum(x.lengths), dtype=torch.float32, device=xin.device), x.lengths)
    sd = torch.tensor(st, dtype=torch.int32, device=xin.device)
    ld = torch.tensor(ls, dtype=torch.int32, device=xin.device)
    check(lib.aware_excerpt_tile(_ptr(xin), _ptr(x.d_off), _ptr(x.d_len), x.B, x.max_len, _ptr(sd), _ptr(ld), _ptr(out.data),
                                 int(bool(adjoint)), _stream()), "aware_excerpt_tile")
    return out


def time_warp(x: Ragged, e, ph, rates, adjoint: bool = False, return_table: bool = False, table=None):
    """Per clip embedding.loop_attacks.time_warp (aware_time_warp): clip b played at a rate that is piecewise linear between
    breakpoints 2^e[b] samples apart, the first one ph[b] samples before the clip's start, with the rate offsets rates[b]
    (integers m_k within -6553..6553, at least warp_breakpoints(len[b], e[b]) of them; the rate is (65536 + m_k) / 65536).  e
    and ph: B integers each, or one for all.  Every clip keeps its length; offsets that are all zero give the identity.  With
    adjoint, x holds the gradient with respect to that output and the result is the gradient with respect to the input.
    return_table: also the table the device built, (R [B, stride] int32, A [B, stride] int64); table: such a pair for the
    adjoint to read, which otherwise reads the one loop_attacks.warp_table gives."""
    from .embedding.loop_attacks import MAX_WARP_DEPTH, MAX_WARP_EXP, MIN_WARP_EXP, warp_breakpoints, warp_table
    lib = load_library()
    es = [int(e)] * x.B if np.isscalar(e) else [int(v) for v in e]
    phs = [int(ph)] * x.B if np.isscalar(ph) else [int(v) for v in ph]
    rs = [np.asarray(r, dtype=np.int64).reshape(-1) for r in rates]
    if len(es) != x.B or len(phs) != x.B or len(rs) != x.B or any(
            not (MIN_WARP_EXP <= eb <= MAX_WARP_EXP and 0 <= pb < (1 << eb) and len(rb) >= warp_breakpoints(n, eb)
                 and np.all(np.abs(rb) <= MAX_WARP_DEPTH)) for eb, pb, rb, n in zip(es, phs, rs, x.lengths)):
        raise ValueError(f"time_warp: per clip {MIN_WARP_EXP} <= e <= {MAX_WARP_EXP}, 0 <= ph < 2^e and ((len + 2^e - 1) >> e) + 2 rate "
                         f"offsets within +-{MAX_WARP_DEPTH} are required; got e = {es}, ph = {phs}, {[len(r) for r in rs]} offsets for "
                         f"lengths {list(x.lengths)}")
    counts = [warp_breakpoints(n, eb) for n, eb in zip(x.lengths, es)]
    stride = max(counts)
    host = np.zeros((x.B, stride), dtype=np.int32)
    for b, (rb, c) in enumerate(zip(rs, counts)):
        host[b, :c] = rb[:c]
    xin = x.data if x.data.dtype == torch.float32 else x.data.float()
    dev = xin.device
    out = Ragged(torch.empty(sum(x.lengths), dtype=torch.float32, device=dev), x.lengths)
    ed = torch.tensor(es, dtype=torch.int32, device=dev)
    pd = torch.tensor(phs, dtype=torch.int32, device=dev)
    rd = torch.from_numpy(host).to(dev)
    if adjoint and table is None:
        tabs = [warp_table(host[b], es[b]) for b in range(x.B)]
        table = (torch.from_numpy(np.stack([t[0] for t in tabs]).astype(np.int32)).to(dev), torch.from_numpy(np.stack([t[1] for t in tabs])).to(dev))
    if adjoint:
        tr, ta = table
        if tr.dtype != torch.int32 or ta.dtype != torch.int64 or tuple(tr.shape) != (x.B, stride) or tuple(ta.shape) != (x.B, stride):
            raise ValueError(f"time_warp: the table is int32 and int64 [{x.B}, {stride}]")
        tr, ta = tr.contiguous(), ta.contiguous()
    else:
        tr = torch.zeros((x.B, stride), dtype=torch.int32, device=dev)
        ta = torch.zeros((x.B, stride), dtype=torch.int64, device=dev)
    check(lib.aware_time_warp(_ptr(xin), _ptr(x.d_off), _ptr(x.d_len), x.B, x.max_len, _ptr(ed), _ptr(pd), _ptr(rd), stride, _ptr(tr),
                              _ptr(ta), _ptr(out.data), int(bool(adjoint)), _stream()), "aware_time_warp")
    return (out, tr, ta) if return_table else out


def gain_envelope(x: Ragged, seeds: Sequence[int], step: int, entry: int, period_samples, floor: float = 0.0,
                  return_gains: bool = False, out: Ragged | None = None):
    """Per clip embedding.loop_attacks.gain_envelope with the draw of chain entry `entry` at optimiser step `step`, always on
    (aware_gain_envelope): clip b times a gain that is piecewise linear between breakpoints P samples apart, P drawn from the
    clip's seed in period_samples = P or (P_lo, P_hi), every breakpoint's gain in [floor, 1].  The operator is its own adjoint.
    out: a Ragged of x's lengths to write into (x itself: in place).  With return_gains the result is (out, gains)."""
    lib = load_library()
    p_lo, p_hi = (int(period_samples),) * 2 if np.isscalar(period_samples) else (int(period_samples[0]), int(period_samples[1]))
    if len(seeds) != x.B:
        raise ValueError(f"gain_envelope: {x.B} clips but {len(seeds)} seeds")
    xin = x.data if x.data.dtype == torch.float32 else x.data.float()
    if out is None:
        out = Ragged(torch.empty(sum(x.lengths), dtype=torch.float32, device=xin.device), x.lengths)
    elif list(out.lengths) != list(x.lengths) or out.data.dtype != torch.float32:
        raise ValueError("gain_envelope: out needs x's lengths in float32")
    gains = Ragged(torch.empty(sum(x.lengths), dtype=torch.float32, device=xin.device), x.lengths) if return_gains else None
    sd = torch.from_numpy(np.array([int(s) & 0xFFFFFFFF for s in seeds], dtype=np.uint32).view(np.int32)).to(xin.device)
    rc = lib.aware_gain_envelope(_ptr(xin), _ptr(x.d_off), _ptr(x.d_len), x.B, x.max_len, _ptr(sd), int(step), int(entry), p_lo, p_hi,
                                 float(floor), _ptr(out.data), _ptr(gains.data) if return_gains else None, _stream())
    if rc == -1:
        raise ValueError(f"gain_envelope: 64 <= P_lo <= P_hi <= 2^20, 0 <= floor < 1, step >= 0 and entry in 0..3 are required; got "
                         f"{p_lo}, {p_hi}, {floor}, step {step}, entry {entry}")
    check(rc, "aware_gain_envelope")
    return (out, gains) if return_gains else out


def band_filter(x: Ragged, response, c1, c2, return_taps: bool = False, out: Ragged | None = None):
    """Per clip embedding.loop_attacks.band_filter (aware_band_filter): clip b through the zero-phase windowed-sinc FIR of 255
    taps with the response bit response[b] (1 lowpass, 2 highpass, 4 bandpass, 8 bandstop) at the edges c1[b] and, for the band
    responses, c2[b], in units of 1 / 65536 cycle per sample (B integers each, or one for all).  Every clip keeps its length,
    zeros are read outside it, and the operator is its own adjoint.  out: a Ragged of x's lengths in float32 to write into, never
    x itself.  With return_taps the result is (out, taps [B, 256] float32: tap k at index k + 127, zero at 255)."""
    lib = load_library()
    rs, a1, a2 = ([int(v)] * x.B if np.isscalar(v) else [int(u) for u in v] for v in (response, c1, c2))
    if (len(rs) != x.B or len(a1) != x.B or len(a2) != x.B or any(r not in (1, 2, 4, 8) for r in rs)
            or any(not 0 <= a <= 32767 for a in a1 + a2) or any(r >= 4 and a > b for r, a, b in zip(rs, a1, a2))):
        raise ValueError(f"band_filter: {x.B} responses of 1, 2, 4, 8 with edges in 0..32767 (c1 <= c2 for a band) are required; "
                         f"got response = {rs}, c1 = {a1}, c2 = {a2}")
    xin = x.data if x.data.dtype == torch.float32 else x.data.float()
    if out is None:
        out = Ragged(torch.empty(sum(x.lengths), dtype=torch.float32, device=xin.device), x.lengths)
    elif list(out.lengths) != list(x.lengths) or out.data.dtype != torch.float32 or out.data.data_ptr() == xin.data_ptr():
        raise ValueError("band_filter: out needs x's lengths in float32 and a buffer of its own")
    taps = torch.zeros((x.B, 256), dtype=torch.float32, device=xin.device) if return_taps else None
    dev = lambda v: torch.tensor(v, dtype=torch.int32, device=xin.device)
    rd, d1, d2 = dev(rs), dev(a1), dev(a2)
    check(lib.aware_band_filter(_ptr(xin), _ptr(x.d_off), _ptr(x.d_len), x.B, x.max_len, _ptr(rd), _ptr(d1), _ptr(d2),
                                _ptr(out.data), _ptr(taps) if return_taps else None, _stream()), "aware_band_filter")
    return (out, taps) if return_taps else out


def frequency_shift(x: Ragged, d, p0, adjoint: bool = False, out: Ragged | None = None):
    """Per clip embedding.loop_attacks.frequency_shift (aware_frequency_shift): clip b moved by d[b] units of sr / 2^20 Hz
    (signed, |d| <= 65536; positive is upwards) from the start phase p0[b] in units of 2^-20 turn, 0 <= p0 < 2^20, through the
    255-tap Hilbert transformer (B integers each, or one for all).  Every clip keeps its length and zeros are read outside it.
    With adjoint, x holds the gradient with respect to that output and the result is the gradient with respect to the input.
    out: a Ragged of x's lengths in float32 to write into, never x itself."""
    from .embedding.loop_attacks import MAX_SHIFT
    lib = load_library()
    ds, ps = ([int(v)] * x.B if np.isscalar(v) else [int(u) for u in v] for v in (d, p0))
    if len(ds) != x.B or len(ps) != x.B or any(abs(v) > MAX_SHIFT for v in ds) or any(not 0 <= v < (1 << 20) for v in ps):
        raise ValueError(f"frequency_shift: {x.B} shifts within +-{MAX_SHIFT} and start phases in [0, 2^20) are required; "
                         f"got d = {ds}, p0 = {ps}")
    xin = x.data if x.data.dtype == torch.float32 else x.data.float()
    if out is None:
        out = Ragged(torch.empty(sum(x.lengths), dtype=torch.float32, device=xin.device), x.lengths)
    elif list(out.lengths) != list(x.lengths) or out.data.dtype != torch.float32 or out.data.data_ptr() == xin.data_ptr():
        raise ValueError("frequency_shift: out needs x's lengths in float32 and a buffer of its own")
    dev = lambda v: torch.tensor(v, dtype=torch.int32, device=xin.device)
    dd, pd = dev(ds), dev(ps)
    check(lib.aware_frequency_shift(_ptr(xin), _ptr(x.d_off), _ptr(x.d_len), x.B, x.max_len, _ptr(dd), _ptr(pd), int(bool(adjoint)),
                                    _ptr(out.data), _stream()), "aware_frequency_shift")
    return out


def sync_select(values: torch.Tensor, n: int, centre: float = 0.0):
    """detection.sync.sync_select on the device (aware_sync_select): values [B * n, L] float32, clip-major, the n candidate
    views of each of the B clips -> (values [B, L] of the view with the largest mean |v - centre| per clip, the smallest j on
    a tie; its index [B] int32; that mean [B] float32)."""
    n = int(n)
    if values.dim() != 2 or n < 1 or values.shape[0] % n or values.shape[0] == 0:
        raise ValueError(f"sync_select: values [B * n, L] with n = {n} are required; got {tuple(values.shape)}")
    v = values.contiguous().float()
    B, L = v.shape[0] // n, v.shape[1]
    out = torch.empty((B, L), dtype=torch.float32, device=v.device)
    idx = torch.empty(B, dtype=torch.int32, device=v.device)
    conf = torch.empty(B, dtype=torch.float32, device=v.device)
    check(load_library().aware_sync_select(_ptr(v), B, n, L, float(centre), _ptr(out), _ptr(idx), _ptr(conf), _stream()),
          "aware_sync_select")
    return out, idx, conf


def _scan_offsets(win_off, what: str):
    """win_off as the C ABI takes it: (host int array [B + 1], B, W); ValueError unless it starts at 0, never falls and
    holds a window."""
    off = [int(o) for o in win_off]
    if len(off) < 2 or off[0] != 0 or off[-1] < 1 or any(b < a for a, b in zip(off, off[1:])):
        raise ValueError(f"{what}: win_off needs B + 1 window offsets from 0 that never fall, with a window in all; got {off}")
    return (C.c_int * len(off))(*off), len(off) - 1, off[-1]


def scan_select(values: torch.Tensor, win_off, n_sync: int, centre: float = 0.0):
    """detection.sync.scan_select on the device (aware_scan_select): values [W * n_sync, L] float32, window-major, the
    n_sync views of each of the W = win_off[-1] windows (win_off: B + 1 host integers, the windows of file b are
    win_off[b] .. win_off[b + 1]) -> (win_values [W, L] float32, win_view [W] int32, win_conf [W] float32, win_bits
    [W, ceil(L / 32)] int32: bit l % 32 of word l // 32 is win_values[w][l] > centre)."""
    n = int(n_sync)
    arr, B, W = _scan_offsets(win_off, "scan_select")
    if values.dim() != 2 or not 1 <= n <= 64 or values.shape[0] != W * n or not 1 <= values.shape[1] <= 512:
        raise ValueError(f"scan_select: values [W * n_sync, L] with W = {W}, n_sync = {n} in 1..64 and L in 1..512 are "
                         f"required; got {tuple(values.shape)}")
    v = values.contiguous().float()
    L = v.shape[1]
    out = torch.empty((W, L), dtype=torch.float32, device=v.device)
    view = torch.empty(W, dtype=torch.int32, device=v.device)
    conf = torch.empty(W, dtype=torch.float32, device=v.device)
    bits = torch.empty((W, (L + 31) // 32), dtype=torch.int32, device=v.device)
    check(load_library().aware_scan_select(_ptr(v), arr, B, n, L, float(centre), _ptr(conf), _ptr(view), _ptr(out), _ptr(bits),
                                           _stream()), "aware_scan_select")
    return out, view, conf, bits


def scan_segments(win_conf: torch.Tensor, win_view: torch.Tensor, win_values: torch.Tensor, win_bits: torch.Tensor, win_off,
                  centre: float, min_confidence: float, max_flip: int, max_segments: int, out=None):
    """detection.sync.scan_segments on the device (aware_scan_segments), on scan_select's four results: per file the runs of
    marked windows that agree on their bits -> {"n_seg" [B] int32: the true run counts; "first", "last", "peak", "view"
    [B, max_segments] int32 (windows counted from the file's first; the peak window's view); "confidence"
    [B, max_segments] float32; "values" [B, max_segments, L] float32}.  Slots beyond a file's runs are not written: they
    hold what `out` (a dict of the same tensors) held, or nothing in particular."""
    arr, B, W = _scan_offsets(win_off, "scan_segments")
    S, L = int(max_segments), int(win_values.shape[-1])
    if (win_values.dim() != 2 or win_values.shape[0] != W or not 1 <= L <= 512 or win_conf.shape != (W,) or win_view.shape != (W,)
            or win_bits.shape != (W, (L + 31) // 32) or S < 1 or int(max_flip) < 0 or not math.isfinite(float(min_confidence))):
        raise ValueError(f"scan_segments: scan_select's results for {W} windows, max_segments >= 1, max_flip >= 0 and a finite "
                         f"min_confidence are required; got values {tuple(win_values.shape)}, max_segments {max_segments}, "
                         f"max_flip {max_flip}, min_confidence {min_confidence}")
    dev = win_values.device
    if out is None:
        out = {k: torch.empty((B, S), dtype=torch.int32, device=dev) for k in ("first", "last", "peak", "view")}
        out.update(n_seg=torch.empty(B, dtype=torch.int32, device=dev),
                   confidence=torch.empty((B, S), dtype=torch.float32, device=dev),
                   values=torch.empty((B, S, L), dtype=torch.float32, device=dev))
    shapes = {"n_seg": (B,), "first": (B, S), "last": (B, S), "peak": (B, S), "view": (B, S), "confidence": (B, S),
              "values": (B, S, L)}
    for k, shp in shapes.items():
        t = out[k]
        if tuple(t.shape) != shp or not t.is_contiguous() or t.device != dev or t.dtype != (
                torch.float32 if k in ("confidence", "values") else torch.int32):
            raise ValueError(f"scan_segments: out[{k!r}] needs the shape {shp}, contiguous, on the values' device")
    tensors = [win_conf.contiguous().float(), win_view.contiguous().int(), win_values.contiguous().float(),
               win_bits.contiguous().int()]
    off_dev = torch.tensor(list(arr), dtype=torch.int32, device=dev)
    check(load_library().aware_scan_segments(*[_ptr(t) for t in tensors], arr, _ptr(off_dev), B, L, float(centre),
                                             float(min_confidence), int(max_flip), S, _ptr(out["n_seg"]), _ptr(out["first"]),
                                             _ptr(out["last"]), _ptr(out["peak"]), _ptr(out["view"]), _ptr(out["confidence"]),
                                             _ptr(out["values"]), _stream()), "aware_scan_segments")
    return out


def viterbi_decode(values: torch.Tensor, centre: float, rate: str, crc: int) -> dict:
    """utils.watermark.fec.viterbi_decode on the device (aware_viterbi_decode): values [R, L] float32, one coded frame per
    row -> {"bits" [R, ceil(T / 32)] int32: the T = L // n decoded input bits, bit t at bit t % 32 of word t // 32
    (fec.unpack_bits); "metric" [R] float32; "valid" [R] bool; "corrected" [R] int32}.  One launch over all rows."""
    from .utils.watermark import fec
    n, c = len(fec.RATES[fec.check_rate(rate)]), fec.check_crc(crc)
    if values.dim() != 2 or not 1 <= values.shape[0] <= fec.MAX_ROWS or not 1 <= values.shape[1] <= fec.MAX_BITS:
        raise ValueError(f"viterbi_decode: values [R, L] with R in 1..{fec.MAX_ROWS} and L in 1..{fec.MAX_BITS} are required; "
                         f"got {tuple(values.shape)}")
    if not math.isfinite(float(centre)):
        raise ValueError(f"viterbi_decode: centre = {centre} is not finite")
    R, L = values.shape
    fec.capacity(L, rate, c)                                      # ValueError where the frame holds no message bit
    v = values.contiguous().float()
    bits = torch.empty((R, (L // n + 31) // 32), dtype=torch.int32, device=v.device)
    metric = torch.empty(R, dtype=torch.float32, device=v.device)
    valid = torch.empty(R, dtype=torch.int32, device=v.device)
    corrected = torch.empty(R, dtype=torch.int32, device=v.device)
    check(load_library().aware_viterbi_decode(_ptr(v), R, L, float(centre), n, c, _ptr(bits), _ptr(metric), _ptr(valid),
                                              _ptr(corrected), _stream()), "aware_viterbi_decode")
    return {"bits": bits, "metric": metric, "valid": valid != 0, "corrected": corrected}


def speed_views(x: Ragged, ms, out: torch.Tensor | None = None):
    """The views of detection.sync's speed search (aware_speed_views): every clip of x at every speed offset of ms, in one
    launch -> (flat float32 device tensor, view lengths, view offsets into it), both clip-major lists of x.B * len(ms); view
    (b, j) is loop_attacks.speed_length(x.lengths[b], ms[j]) samples, bit for bit speed_change(x, ms[j]) at that length.  The
    offsets are multiples of four floats; the up to three floats between two rows are not written.  out: a float32 device
    tensor of at least the views' size to write into."""
    from .embedding.loop_attacks import speed_length
    lib = load_library()
    ms = [int(v) for v in ms]
    if not 1 <= len(ms) <= 63 or any(v < -13520 or v > 17034 for v in ms):
        raise ValueError(f"speed_views: 1 to 63 speed offsets within -13520..17034 (-+400 cents) are required; got {ms}")
    if min(x.lengths) < 1:
        raise ValueError(f"speed_views: every clip needs a sample; got {x.lengths}")
    vlen = [speed_length(n, m) for n in x.lengths for m in ms]
    voff = np.concatenate([[0], np.cumsum([(n + 3) // 4 * 4 for n in vlen])]).astype(np.int64)
    if int(voff[-1]) > 1 << 30:
        raise ValueError(f"speed_views: the views hold {int(voff[-1])} samples; at most 2^30 per call")
    xin = x.data if x.data.dtype == torch.float32 else x.data.float()
    if out is None:
        flat = torch.empty(int(voff[-1]), dtype=torch.float32, device=xin.device)
    elif out.dtype != torch.float32 or out.dim() != 1 or out.numel() < int(voff[-1]) or not out.is_contiguous() or out.device != xin.device:
        raise ValueError(f"speed_views: out needs {int(voff[-1])} contiguous float32 values on x's device")
    else:
        flat = out
    md = torch.tensor(ms, dtype=torch.int32, device=xin.device)
    od = torch.tensor(voff[:-1], dtype=torch.int32, device=xin.device)
    check(lib.aware_speed_views(_ptr(xin), _ptr(x.d_off), _ptr(x.d_len), x.B, _ptr(md), len(ms), _ptr(flat), _ptr(od),
                                max(vlen), _stream()), "aware_speed_views")
    return flat, vlen, voff[:-1].tolist()


def shift_views(x: Ragged, d, out: torch.Tensor | None = None):
    """The views of detection.sync's shift search (aware_shift_views): every clip of x at every frequency shift of d (units of
    sr / 2^20 Hz, signed, |d| <= 65536), in one launch -> (flat float32 device tensor, view lengths, view offsets into it),
    both clip-major lists of x.B * len(d); view (b, j) is x.lengths[b] samples, bit for bit frequency_shift(x, d[j], 0).  The
    offsets are multiples of four floats; the up to three floats between two rows are not written.  out: a float32 device
    tensor of at least the views' size to write into."""
    from .embedding.loop_attacks import MAX_SHIFT
    lib = load_library()
    ds = [int(v) for v in d]
    if not 1 <= len(ds) <= 63 or any(abs(v) > MAX_SHIFT for v in ds):
        raise ValueError(f"shift_views: 1 to 63 shifts within +-{MAX_SHIFT} are required; got {ds}")
    if min(x.lengths) < 1:
        raise ValueError(f"shift_views: every clip needs a sample; got {x.lengths}")
    vlen = [int(n) for n in x.lengths for _ in ds]
    voff = np.concatenate([[0], np.cumsum([(n + 3) // 4 * 4 for n in vlen])]).astype(np.int64)
    if int(voff[-1]) > 1 << 30:
        raise ValueError(f"shift_views: the views hold {int(voff[-1])} samples; at most 2^30 per call")
    xin = x.data if x.data.dtype == torch.float32 else x.data.float()
    if out is None:
        flat = torch.empty(int(voff[-1]), dtype=torch.float32, device=xin.device)
    elif out.dtype != torch.float32 or out.dim() != 1 or out.numel() < int(voff[-1]) or not out.is_contiguous() or out.device != xin.device:
        raise ValueError(f"shift_views: out needs {int(voff[-1])} contiguous float32 values on x's device")
    else:
        flat = out
    dd = torch.tensor(ds, dtype=torch.int32, device=xin.device)
    od = torch.tensor(voff[:-1], dtype=torch.int32, device=xin.device)
    check(lib.aware_shift_views(_ptr(xin), _ptr(x.d_off), _ptr(x.d_len), x.B, _ptr(dd), len(ds), _ptr(flat), _ptr(od),
                                max(vlen), _stream()), "aware_shift_views")
    return flat, vlen, voff[:-1].tolist()


def stretch_ola(x: Ragged, m, adjoint: bool = False, out_lengths=None) -> Ragged:
    """Per clip embedding.loop_attacks.time_stretch at the offsets m (B integers, or one for all): clip b stretched in time at
    the rate (65536 + m[b]) / 65536 by plain overlap-add (aware_stretch_ola), out_lengths[b] samples long (default: the clip's
    own length).  With adjoint, x holds the gradient with respect to that output and the result, out_lengths long, is the
    gradient with respect to the input (out_lengths is then the forward pass's input lengths)."""
    return _resample_alone("stretch_ola", "aware_stretch_ola", -16384, 21845, "offsets within -16384..21845 (rates 0.75 to 4/3)",
                           x, m, adjoint, out_lengths)


def pitch_shift_ola(x: Ragged, m, adjoint: bool = False, out_lengths=None) -> Ragged:
    """Per clip embedding.loop_attacks.pitch_shift at the speed offsets m (B integers, or one for all): clip b with its pitch
    moved by the ratio (65536 + m[b]) / 65536 at its own duration, the overlap-add stretch at the coupled rate and the
    resampling in one launch (aware_pitch_shift_ola), out_lengths[b] samples long (default: the clip's own length).  With
    adjoint, x holds the gradient with respect to that output and the result, out_lengths long, is the gradient with respect to
    the input (out_lengths is then the forward pass's input lengths)."""
    return _resample_alone("pitch_shift_ola", "aware_pitch_shift_ola", -13520, 17034, "speed offsets within -13520..17034 (-+400 cents)",
                           x, m, adjoint, out_lengths)


PV_MQ_MIN, PV_MQ_MAX = -16384, 21845       # the stretch's range: ceil / floor of 65536 (0.75 - 1) and 65536 (4 / 3 - 1)


def _pv_args(B: int, frame_offsets, mq, dev, who: str):
    mqs = [int(mq)] * B if np.isscalar(mq) else [int(v) for v in mq]
    if len(mqs) != B or any(v < PV_MQ_MIN or v > PV_MQ_MAX for v in mqs):
        raise ValueError(f"{who}: {B} stretch offsets within {PV_MQ_MIN}..{PV_MQ_MAX} (rates 0.75 to 4/3) are required; got {mqs}")
    fo = [int(v) for v in frame_offsets]
    if len(fo) != B + 1 or fo[0] < 0 or any(b <= a for a, b in zip(fo, fo[1:])):
        raise ValueError(f"{who}: {B + 1} ascending frame offsets are required; got {fo}")
    return torch.tensor(fo, dtype=torch.int32, device=dev), torch.tensor(mqs, dtype=torch.int32, device=dev), fo


def pv_frames(spec: torch.Tensor, frame_offsets, mq) -> torch.Tensor:
    """embedding.loop_attacks.pv_frames per clip on a ragged spectrum (aware_pv_frames): spec [rows, 520] complex64 as `stft`
    writes it, clip b's frames at rows frame_offsets[b] .. frame_offsets[b + 1] (B + 1 values; rows outside them are left
    alone), mq B stretch offsets or one for all.  mq[b] = 0 copies the clip's rows."""
    B = len(frame_offsets) - 1
    fo, md, host = _pv_args(B, frame_offsets, mq, spec.device, "pv_frames")
    if spec.dtype != torch.complex64 or spec.dim() != 2 or spec.shape[1] != FULL_STRIDE or spec.shape[0] < host[-1] or not spec.is_contiguous():
        raise ValueError(f"pv_frames: a contiguous complex64 spectrum [>= {host[-1]}, {FULL_STRIDE}] is required")
    out = torch.zeros_like(spec)
    check(load_library().aware_pv_frames(_ptr(spec), _ptr(fo), B, _ptr(md), _ptr(out), _stream()), "aware_pv_frames")
    return out


def pv_frames_bwd(spec: torch.Tensor, grad_out: torch.Tensor, frame_offsets, mq) -> torch.Tensor:
    """Backward of `pv_frames` through the magnitudes (aware_pv_frames_bwd; the phases are constants): the gradient with respect
    to spec from grad_out, the gradient with respect to pv_frames' result; both laid out as spec."""
    B = len(frame_offsets) - 1
    fo, md, host = _pv_args(B, frame_offsets, mq, spec.device, "pv_frames_bwd")
    for t in (spec, grad_out):
        if t.dtype != torch.complex64 or t.dim() != 2 or t.shape[1] != FULL_STRIDE or t.shape[0] < host[-1] or not t.is_contiguous():
            raise ValueError(f"pv_frames_bwd: contiguous complex64 spectra [>= {host[-1]}, {FULL_STRIDE}] are required")
    out = torch.zeros_like(spec)
    check(load_library().aware_pv_frames_bwd(_ptr(spec), _ptr(grad_out), _ptr(fo), B, _ptr(md), _ptr(out), _stream()),
          "aware_pv_frames_bwd")
    return out


def pv_stretch(plan: "Plan", x: Ragged, mq) -> Ragged:
    """Per clip embedding.loop_attacks.pv_stretch at the stretch offsets mq (B integers, or one for all): STFT -> pv_frames ->
    iSTFT on the card geometry, every clip as long as it was (the iSTFT gives 256 (n // 256) samples, zeros follow; a clip with
    mq[b] = 0 is returned as it is).  ValueError for an mq outside the stretch's range."""
    mqs = [int(mq)] * x.B if np.isscalar(mq) else [int(v) for v in mq]
    if len(mqs) != x.B or any(v < PV_MQ_MIN or v > PV_MQ_MAX for v in mqs):          # before any launch
        raise ValueError(f"pv_stretch: {x.B} stretch offsets within {PV_MQ_MIN}..{PV_MQ_MAX} (rates 0.75 to 4/3) are required; got {mqs}")
    bt = Batch(x.lengths)
    xin = x.data if x.data.dtype == torch.float32 else x.data.float()
    y = istft(plan, bt, pv_frames(stft(plan, bt, xin, normalize=False), bt.frame_offsets, mqs), normalize=False)
    out = Ragged(torch.zeros_like(xin), x.lengths)
    for b in range(x.B):
        o, n = out.offsets[b], (x.lengths[b] if mqs[b] == 0 else bt.out_lengths[b])
        out.data[o:o + n] = xin[o:o + n] if mqs[b] == 0 else y[bt.out_offsets[b]: bt.out_offsets[b] + n]
    return out


def phase_vocoder_frames(frames: Sequence[int], rate: float):
    """Frames per clip after a phase vocoder at `rate`: len(np.arange(0, T, rate))."""
    return [int(len(np.arange(0, int(t), float(rate)))) for t in frames]


def time_stretch(plan: "Plan", x: Ragged, rate: float) -> Ragged:
    """STFT -> phase vocoder -> iSTFT of every clip (EXTENSION, see aware_phase_vocoder).  Output length
    256*(ceil(T/rate) - 1) samples per clip."""
    lib = load_library()
    dev = x.data.device
    bin_ = Batch(x.lengths)
    spec = stft(plan, bin_, x.data if x.data.dtype == torch.float32 else x.data.float(), normalize=False)
    to = phase_vocoder_frames(bin_.frames, rate)
    if min(to) < 3:
        raise ValueError("time_stretch: a clip would shrink below 3 frames")
    bout = Batch([256 * (t - 1) + 1 for t in to])                    # a batch whose clips have exactly `to` frames
    assert bout.frames == to
    fin = torch.tensor(bin_.frame_offsets, dtype=torch.int32, device=dev)
    fout = torch.tensor(bout.frame_offsets, dtype=torch.int32, device=dev)
    out_spec = torch.empty((bout.total_frames, FULL_STRIDE), dtype=torch.complex64, device=dev)
    check(lib.aware_phase_vocoder(_ptr(spec), _ptr(fin), _ptr(out_spec), _ptr(fout), x.B, float(rate), _stream()),
          "aware_phase_vocoder")
    y = istft(plan, bout, out_spec, normalize=False)
    return Ragged(y, bout.out_lengths)


def snr_db(output: Ragged, target: Ragged) -> torch.Tensor:
    """Per-clip SNR in dB of `output` against `target` over the common length (metrics/audio.py:68-89);
    device float64 tensor [B]."""
    if output.B != target.B:
        raise ValueError("snr_db: batches differ in size")
    lib = load_library()
    dev = output.data.device
    n = torch.minimum(output.d_len, target.d_len)
    out = torch.empty(output.B, dtype=torch.float64, device=dev)
    check(lib.aware_snr(_ptr(output.data), _ptr(output.d_off), _ptr(target.data), _ptr(target.d_off), _ptr(n), output.B,
                        _ptr(out), _stream()), "aware_snr")
    return out


STOI_FS = 10000
_STOI_CACHE = {}


def stoi_frames(n: int) -> int:
    """First-stage frames of a clip of n samples at 10 kHz: len(range(0, n - 256, 128)) -- the device's arithmetic."""
    return (n - 256 + 127) // 128 if n > 256 else 0


def stoi_reframed(kept: int) -> int:
    """Frames of the signal rebuilt from `kept` frames by overlap-add: kept - 1 (none for kept <= 1)."""
    return max(kept - 1, 0)


def stoi_segments(kept: int) -> int:
    """30-frame segments of a clip with `kept` frames; 0 means the score is 1e-5."""
    return max(stoi_reframed(kept) - 29, 0)


def stoi_resample_filter(sample_rate: int):
    """What metrics.audio._resample_oct hands to scipy.signal.resample_poly for sample_rate -> 10 kHz: the Kaiser-windowed
    sinc normalised to unit sum and (inside resample_poly) scaled by `up`; float32 taps, up, down, half length."""
    from .metrics.audio import _resample_window_oct
    g = int(np.gcd(STOI_FS, int(sample_rate)))
    up, down = STOI_FS // g, int(sample_rate) // g
    h = _resample_window_oct(STOI_FS, int(sample_rate))
    h = h / np.sum(h) * up
    return h.astype(np.float32), up, down, (len(h) - 1) // 2


class _StoiPlan:
    def __init__(self):
        require_gpu()
        self.h = C.c_void_p()
        check(load_library().aware_stoi_create(C.byref(self.h)), "aware_stoi_create")

    def __del__(self):
        try:
            if self.h:
                load_library().aware_stoi_destroy(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass


def _stoi_plan(dev) -> "_StoiPlan":
    key = ("plan", str(dev))
    if key not in _STOI_CACHE:
        _STOI_CACHE[key] = _StoiPlan()
    return _STOI_CACHE[key]


def _stoi_filter(sample_rate: int, dev):
    key = ("fir", int(sample_rate), str(dev))
    if key not in _STOI_CACHE:
        h, up, down, half = stoi_resample_filter(sample_rate)
        _STOI_CACHE[key] = (torch.from_numpy(h).to(dev), up, down, half)
    return _STOI_CACHE[key]


def stoi(output: Ragged, target: Ragged, sample_rate: int = 16000, return_kept: bool = False):
    """Short-time objective intelligibility of every clip of `output` (the processed signal) against `target` (the clean
    one) over their common length: the function `metrics.audio.stoi(target, output, sample_rate)` computes on the host,
    on the device for the whole batch (argument order of `snr_db` and of the reference's STOI.__call__,
    metrics/audio.py:42-64).  Both batches are resampled to 10 kHz with the polyphase kernel (`sample_rate == 10000`
    skips that).  Device float64 tensor [B]; with return_kept also the kept-frame count of every clip (device int32)."""
    if output.B != target.B:
        raise ValueError("stoi: batches differ in size")
    lib = load_library()
    dev = output.data.device
    B = output.B
    n_in = [min(a, b) for a, b in zip(output.lengths, target.lengths)]
    pr = output.data if output.data.dtype == torch.float32 else output.data.float()
    cl = target.data if target.data.dtype == torch.float32 else target.data.float()
    p_off, c_off = output.d_off, target.d_off
    if int(sample_rate) != STOI_FS:
        h, up, down, half = _stoi_filter(sample_rate, dev)
        n10 = [-(-n * up // down) for n in n_in]
        d_in = torch.tensor(n_in, dtype=torch.int32, device=dev)
        off10 = np.concatenate([[0], np.cumsum(n10)[:-1]]).astype(np.int32)
        d_off10 = torch.from_numpy(off10).to(dev)
        d_n = torch.tensor(n10, dtype=torch.int32, device=dev)
        res = torch.empty((2, max(sum(n10), 1)), dtype=torch.float32, device=dev)
        for src, off, dst in ((cl, c_off, res[0]), (pr, p_off, res[1])):
            check(lib.aware_upfirdn(_ptr(src), _ptr(off), _ptr(d_in), _ptr(dst), _ptr(d_off10), _ptr(d_n), B, max(n10),
                                    _ptr(h), h.numel(), up, down, half, _stream()), "aware_upfirdn")
        cl, pr, c_off, p_off = res[0], res[1], d_off10, d_off10
    else:
        n10 = n_in
        d_n = torch.tensor(n10, dtype=torch.int32, device=dev)
    max_len, total = max(n10), max(sum(n10), max(n10))
    plan = _stoi_plan(dev)
    nbytes = lib.aware_stoi_workspace_bytes(B, max_len, total)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(B, dtype=torch.float64, device=dev)
    kept = torch.empty(B, dtype=torch.int32, device=dev) if return_kept else None
    check(lib.aware_stoi(plan.h, _ptr(cl), _ptr(c_off), _ptr(pr), _ptr(p_off), _ptr(d_n), B, max_len, total, _ptr(out),
                         _ptr(kept), _ptr(ws), nbytes, _stream()), "aware_stoi")
    return (out, kept) if return_kept else out


KERNEL_KINDS = ["synth", "analysis", "gemm_nt", "mel_norm", "in_lrelu", "readout_tail", "synth_adjoint",
                "analysis_adjoint_nadam", "misc", "gemm_clip_fwd", "gemm_clip_bwd", "gemm_x3_fwd", "gemm_x3_bwd"]


def embed_profile(sess: EmbedSession, n_iters: int = 3):
    """Per-launch milliseconds of `n_iters` eager loop bodies, measured with HIP events recorded
    on the launch stream (aware_embed_profile).  Returns a list of (kind_name, ms)."""
    cap = 64 * n_iters
    ms = (C.c_float * cap)()
    kind = (C.c_int * cap)()
    n = sess.lib.aware_embed_profile(sess.h, n_iters, cap, ms, kind, _stream())
    if n < 0:
        check(n, "aware_embed_profile")
    return [(KERNEL_KINDS[kind[i]], float(ms[i])) for i in range(n)]


def spectral_quantize(spec: torch.Tensor, step_db: float, floor_db: float) -> torch.Tensor:
    """in place on a [frames, 520] complex64 spectrum (EXTENSION: MP3-like surrogate)"""
    lib = load_library()
    check(lib.aware_spectral_quantize(_ptr(spec), spec.shape[0], float(step_db), float(floor_db), _stream()),
          "aware_spectral_quantize")
    return spec


def spectral_quantize_bwd(spec_in: torch.Tensor, grad_out: torch.Tensor, step_db: float, floor_db: float) -> torch.Tensor:
    """Backward of the surrogate (straight-through on the magnitude, exact through the phase); spec_in: the spectrum before
    quantisation."""
    lib = load_library()
    gin = torch.empty_like(spec_in)
    go = grad_out.contiguous()
    check(lib.aware_spectral_quantize_bwd(_ptr(spec_in), _ptr(go), _ptr(gin), spec_in.shape[0], float(step_db), float(floor_db),
                                          _stream()), "aware_spectral_quantize_bwd")
    return gin


class SpectralQuantizeSTE(torch.autograd.Function):
    """The MP3-like surrogate as a differentiable torch op on a [frames, 520] complex64 spectrum (aware_spectral_quantize /
    aware_spectral_quantize_bwd)."""

    @staticmethod
    def forward(ctx, spec, step_db, floor_db):
        ctx.save_for_backward(spec)
        ctx.step_db, ctx.floor_db = float(step_db), float(floor_db)
        return spectral_quantize(spec.detach().clone(), step_db, floor_db)

    @staticmethod
    def backward(ctx, grad_out):
        (spec,) = ctx.saved_tensors
        return spectral_quantize_bwd(spec, grad_out, ctx.step_db, ctx.floor_db), None, None
