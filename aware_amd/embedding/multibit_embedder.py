"""AWAREEmbedder: per-clip adversarial optimisation of the in-band STFT magnitudes against the
frozen detector, batched over clips on the GPU.

Reference: src/AWARE/embedding/multibit_embedder.py:17-197.  embed() keeps the reference's
signature and return value (normalised waveform of 256*(T-1) samples); embed_batch() is the
MI355X entry point: any number of ragged clips, one optimisation problem each, all iterations
enqueued without host synchronisation."""
from __future__ import annotations

import time

import numpy as np
import torch

from ..detection import AWAREDetectorNet
from ..interfaces import BaseEmbedder
from ..utils.audio import ISTFT, STFT, STFTAssembler, STFTDecomposer, WaveformNormalizer, band_bins, get_plan
from ..utils.logger import logger
from .. import runtime as rt
from ..utils.watermark import fec
from .loop_attacks import parse_chain, parse_mixture
from .losses import get_loss_fn
from .optimizers import get_optimizer, is_card_default
from .schedulers import get_scheduler


class AWAREEmbedder(BaseEmbedder):
    def __init__(self, frame_length: int = 1024, hop_length: int = 256, window: str = "hann", win_length: int = 1024,
                 pattern_mode: str = "bits2bipolar", embedding_bands=(500, 4000), tolerance_db: float = 6.0,
                 num_iterations: int = 400, detection_net_cfg: dict = None, optimizer_cfg: dict = None,
                 scheduler_cfg: dict = None, loss: str = "push", verbose: bool = True, use_graph: bool = True,
                 loop_attacks=None, loop_attack_seed: int = 0, loop_attack_mixture=None, payload_code=None,
                 general_geometry: bool = False, temporal_convs: bool = False, initial_pools: bool = False,
                 general_loop_attacks: bool = False):
        """loop_attacks (EXTENSION, see embedding/loop_attacks.py): a chain of attacks applied inside the optimisation loop,
        e.g. [{"kind": "gaussian_noise", "snr_db": 10.0}, {"kind": "sample_suppression", "seconds": 0.3, "prob": 0.75}];
        clip i of a batch draws with seed loop_attack_seed + i.  None: the reference's loop (clean synthesis only).
        loop_attack_mixture (EXTENSION): a list of {"weight": w, "chain": [...]}; every clip draws one of the chains (or, with
        what the weights leave of 1, none) afresh at every step, so one watermark meets several attack families.  Giving
        both loop_attacks and loop_attack_mixture is a ValueError.
        payload_code (EXTENSION, utils/watermark/fec.py): {"rate": "1/2" or "1/3", "crc": 0, 8 or 16}, the channel code of
        service.embed_message; None: no code.  embed() itself is not changed by it.
        general_geometry (EXTENSION): embed at any frame_length in runtime.GENERAL_NFFT, any
        hop_length and win_length in 1..frame_length, on the general route (the card geometry included); off: the card
        geometry only, on the card kernels.  With it, loop_attacks, loop_attack_mixture and the loss push_extremes_l1 raise
        NotImplementedError, and detection_net_cfg.n_fft has to equal frame_length.
        general_loop_attacks (EXTENSION): beside general_geometry, loop_attacks may hold up to four
        entries of the kinds that do not split a chain (runtime.GENERAL_CHAIN_KINDS: gaussian_noise, sample_suppression,
        gain_envelope), in any order, and the session runs them on the general route; every other kind and
        loop_attack_mixture still raise NotImplementedError.  Without general_geometry the key changes nothing.
        temporal_convs (EXTENSION): handed to the detection net built from detection_net_cfg, where it
        opens kernel_size / stride / padding other than 1 / 1 / 0 (AWAREDetectorNet); off: 1x1 convolutions only.
        initial_pools (EXTENSION): handed to the detection net in the same way, where it opens
        initial_pool_size / initial_pool_stride 2..8; off: the (2, 2) pool only."""
        self.general_geometry = bool(general_geometry)
        rt.require_card_geometry("AWAREEmbedder", frame_length, hop_length, win_length, self.general_geometry, window)
        self.frame_length, self.hop_length, self.window, self.win_length = frame_length, hop_length, window, win_length
        self.device = torch.device("cuda")
        self.embedding_bands = tuple(embedding_bands)
        self.tolerance_db = tolerance_db
        self.num_iterations = num_iterations
        self.pattern_mode = pattern_mode
        self.temporal_convs = bool(temporal_convs)
        net_cfg = dict(detection_net_cfg or {})
        if self.temporal_convs:
            net_cfg["temporal_convs"] = True
        self.initial_pools = bool(initial_pools)
        if self.initial_pools:
            net_cfg["initial_pools"] = True
        self.detection_net = AWAREDetectorNet(**net_cfg)
        self.detection_net.embedding_bands = self.embedding_bands
        if self.general_geometry and self.detection_net.n_fft != frame_length:
            # the mel bank is [n_mels, n_fft/2 + 1] and multiplies spectra of frame_length/2 + 1 bins
            raise ValueError(f"AWAREEmbedder: detection_net_cfg.n_fft = {self.detection_net.n_fft} but frame_length = "
                             f"{frame_length}; with general_geometry the detector's mel bank follows the STFT")
        self.payload_code = fec.check_payload_code(payload_code)      # ValueError naming the key
        if self.payload_code:
            fec.capacity(self.detection_net.output_length, **self.payload_code)   # ValueError where no message bit is left
        optimizer_cfg = optimizer_cfg or {"name": "nadam", "params": {"lr": 0.1}}
        scheduler_cfg = scheduler_cfg or {"name": "reduce_lr_on_plateau", "params": {"factor": 0.9, "patience": 500}}
        self.optimizer_name, self.optimizer_params = optimizer_cfg["name"], optimizer_cfg.get("params", {}) or {}
        self.scheduler_name, self.scheduler_params = scheduler_cfg["name"], scheduler_cfg.get("params", {}) or {}
        # ValueError on an unknown name, as the reference; bce on a detector that does not end in sigmoid raises here
        # (NotImplementedError), where the reference raises inside torch at the first step
        self.loss = get_loss_fn(loss, final_activation=self.detection_net.final_activation)
        if self.general_geometry and getattr(self.loss, "l1_weight", 0.0):
            rt.refuse_general_geometry("the loss push_extremes_l1 (its L1 term lives in the streaming kernels)")
        self._opt = get_optimizer(self.optimizer_name, None, **self.optimizer_params)
        self._sched = get_scheduler(self.scheduler_name, self._opt, num_iterations, **self.scheduler_params)
        self.verbose = verbose
        self.use_graph = use_graph
        self.loop_attacks = parse_chain(loop_attacks)     # ValueError on an unknown kind / key, prob outside [0, 1], > 4 entries
        self.loop_attack_mixture = parse_mixture(loop_attack_mixture)      # ValueError with the index of the offending chain
        if self.loop_attacks and self.loop_attack_mixture:
            raise ValueError("AWAREEmbedder: loop_attacks or loop_attack_mixture, not both")
        self.general_loop_attacks = bool(general_loop_attacks)
        if self.general_geometry and self.loop_attacks:
            if not self.general_loop_attacks:
                rt.refuse_general_geometry("loop_attacks", "; the key general_loop_attacks opens the kinds "
                                           + ", ".join(rt.GENERAL_CHAIN_KINDS) + " on the general route")
            rt.check_general_chain(self.loop_attacks)
        if self.general_geometry and self.loop_attack_mixture:
            rt.refuse_general_geometry("loop_attack_mixture")
        self.loop_attack_seed = int(loop_attack_seed)
        self.conv_pipe = "f16x2"                       # runtime.CONV_PIPES: arithmetic of the detector's conv-block GEMMs
        self.conv_tile = "auto"                        # runtime.CONV_TILES: form of the f16 two-term conv kernel (same bits)
        self.audio_preprocess_pipeline = [WaveformNormalizer(), STFT(frame_length, hop_length, window, win_length), STFTDecomposer()]
        self.audio_postprocess_pipeline = [STFTAssembler(), ISTFT(frame_length, hop_length, window, win_length), WaveformNormalizer()]

    # ---- geometry ---------------------------------------------------------------------------
    def _get_embedding_frequency_indices(self, sampling_rate: int, frame_length: int):
        lo, hi = band_bins(sampling_rate, frame_length, self.embedding_bands)
        allb = np.arange(1 + frame_length // 2)
        mask = (allb >= lo) & (allb <= hi)
        return allb[mask], allb[~mask]

    def _plan(self, sample_rate):
        rt.require_card_geometry("AWAREEmbedder", self.frame_length, self.hop_length, self.win_length, self.general_geometry,
                                 self.window)
        return get_plan(self.frame_length, self.hop_length, self.window,
                        band_bins(sample_rate, self.frame_length, self.embedding_bands), win_length=self.win_length,
                        general=self.general_geometry)

    def check_clips(self, lengths):
        """With general_geometry: ValueError naming the first clip the geometry cannot embed (runtime.check_general_clips: too
        short, NOLA); needs no GPU.  Without the key the card batch checks its clips itself."""
        if self.general_geometry:
            rt.check_general_clips("AWAREEmbedder", self.frame_length, self.hop_length, self.win_length, self.window, lengths)
        # a net of temporal convolutions: every clip keeps a row through every block (T = 1 + n // hop frames)
        self.detection_net.check_clip_frames("AWAREEmbedder", [1 + int(n) // self.hop_length for n in lengths])

    def check_targets(self, watermarks):
        """With the loss bce: ValueError for a target outside [0, 1], as F.binary_cross_entropy refuses one (the device would
        take it without a word); needs no GPU.  embed and embed_batch call it before anything is launched; embed_device takes
        device targets as they are."""
        if self.loss.name != "bce":
            return
        wm = np.asarray(watermarks, dtype=np.float32)
        if not np.all((wm >= 0.0) & (wm <= 1.0)):            # a NaN fails it too
            raise ValueError("AWAREEmbedder: the loss bce takes targets between 0 and 1 (pattern_mode bytes2bits), got values "
                             f"from {np.nanmin(wm)} to {np.nanmax(wm)}")

    def make_batch(self, lengths, sample_rate: int) -> "rt.Batch":
        """The batch geometry of this embedder's plan for clips of `lengths` samples."""
        self.check_clips(lengths)
        return rt.Batch(list(lengths), plan=self._plan(sample_rate) if self.general_geometry else None)

    # ---- batched hot path ----------------------------------------------------------------------
    def start_session(self, batch: "rt.Batch", sample_rate: int, attack_seeds=None) -> "rt.EmbedSession":
        sess = self._start_session(batch, sample_rate)
        if self.loop_attacks and self.general_geometry:
            seeds = attack_seeds if attack_seeds is not None else [self.loop_attack_seed + i for i in range(batch.B)]
            sess.set_general_chain(self.loop_attacks, seeds, sample_rate)
        elif self.loop_attacks:
            seeds = attack_seeds if attack_seeds is not None else [self.loop_attack_seed + i for i in range(batch.B)]
            sess.set_loop_attacks(self.loop_attacks, seeds, sample_rate)
        elif self.loop_attack_mixture:
            seeds = attack_seeds if attack_seeds is not None else [self.loop_attack_seed + i for i in range(batch.B)]
            sess.set_loop_mixture(self.loop_attack_mixture, seeds, sample_rate)
        return sess

    def _start_session(self, batch: "rt.Batch", sample_rate: int) -> "rt.EmbedSession":
        plan = self._plan(sample_rate)
        common = dict(num_iterations=self.num_iterations, tolerance_db=self.tolerance_db, loss=self.loss.name,
                      use_graph=self.use_graph, l1_weight=getattr(self.loss, "l1_weight", 0.0), conv_pipe=self.conv_pipe,
                      conv_tile=self.conv_tile)
        det = self.detection_net.device_weights(plan)
        if is_card_default(self._opt) and self._sched["constant_lr"]:
            # the model card's configuration (NAdam, a scheduler that cannot fire): fused in the adjoint kernel's epilogue
            g = self._opt["group"]
            return rt.EmbedSession(plan, det, batch, lr=g["lr"], beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"],
                                   momentum_decay=g["momentum_decay"], **common)
        # any other registry entry (embedding/optimizers.py:3-20, schedulers.py:3-16): per-step scalars from the host.  The
        # scheduler object is consumed by building the table, so each session gets fresh ones
        opt = get_optimizer(self.optimizer_name, None, **self.optimizer_params)
        sched = get_scheduler(self.scheduler_name, opt, self.num_iterations, **self.scheduler_params)
        sess = rt.EmbedSession(plan, det, batch, **common)
        sess.set_optimizer(opt, sched)
        return sess

    def embed_device(self, audio: torch.Tensor, batch: "rt.Batch", sample_rate: int, watermarks: torch.Tensor,
                     rescale: torch.Tensor | None = None, session: "rt.EmbedSession" = None, attack_seeds=None):
        """audio: device f32 ragged at batch.in_offsets; watermarks: device [B, n_bits] bipolar.
        attack_seeds: per-clip seeds of the loop attacks (default loop_attack_seed + clip index; a session passed in keeps
        the seeds it was started with).  Returns (flat device output at batch.out_offsets, session)."""
        sess = session or self.start_session(batch, sample_rate, attack_seeds)
        sess.begin(audio, watermarks)
        sess.iterate(self.num_iterations)
        return sess.finish(rescale), sess

    def embed_batch(self, clips, sample_rate: int, watermarks, rescale=None):
        """clips: list of 1-D float arrays; watermarks: [B, n_bits] bipolar (0 / 1 for the unipolar losses).  Returns a list of
        device tensors (one per clip, length hop_length*(T_b-1) with T_b = 1 + n_b // hop_length)."""
        t0 = time.time()
        self.check_targets(watermarks)
        batch = self.make_batch([len(c) for c in clips], sample_rate)
        wm = torch.as_tensor(np.asarray(watermarks), dtype=torch.float32, device="cuda")
        rs = None if rescale is None else torch.as_tensor(np.asarray(rescale), dtype=torch.float32, device="cuda")
        out, sess = self.embed_device(batch.pack(clips), batch, sample_rate, wm, rs)
        if self.verbose:
            torch.cuda.synchronize()
            logger.info(f"Optimization completed in {time.time() - t0:.1f}s after {self.num_iterations} iterations")
            logger.info(f"Final loss: {float(sess.best_loss.mean()):.6f}")
        return batch.unpack_out(out)

    # ---- reference-shaped single-clip entry ------------------------------------------------------
    def embed(self, audio: np.ndarray, sample_rate: int, watermark: np.ndarray) -> np.ndarray:
        try:
            out = self.embed_batch([np.asarray(audio, dtype=np.float32)], sample_rate,
                                   np.asarray(watermark, dtype=np.float32)[None])
        except Exception as exc:
            logger.error(f"Error during embedding: {exc}")
            raise
        return out[0].detach().cpu().numpy()
