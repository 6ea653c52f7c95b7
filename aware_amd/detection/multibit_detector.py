"""AWAREDetector.detect on the HIP path.

Reference: src/AWARE/detection/multibit_detector.py:9-42 -- normalise, STFT, magnitude, zero the
bins outside the embedding band, network forward.  Batched entry point: detect_batch.  EXTENSION: sync_search = n reads n views of every clip, 512 / n samples
apart, and keeps the most confident one (detection/sync.py); off by default."""
from __future__ import annotations

import numpy as np
import torch

from ..interfaces import BaseDetector
from ..utils.audio import STFT, STFTDecomposer, WaveformNormalizer, band_bins, get_plan
from .. import runtime as rt
from . import sync


class AWAREDetector(BaseDetector):
    def __init__(self, model, threshold: float = 0.0, frame_length: int = 1024, hop_length: int = 256,
                 window: str = "hann", win_length: int = 1024, pattern_mode: str = "bits2bipolar",
                 embedding_bands=(500, 4000), sync_search: int = 0):
        rt.require_card_geometry("AWAREDetector", frame_length, hop_length, win_length)
        self.sync_search = sync.check_sync_search(sync_search)
        self.threshold = threshold
        self.device = torch.device("cuda")
        self.pattern_mode = pattern_mode
        self.embedding_bands = tuple(embedding_bands)
        self.win_length = win_length
        self.frame_length = frame_length
        self.hop_length = hop_length
        self.window = window
        self.detection_net = model
        self.audio_preprocess_pipeline = [WaveformNormalizer(), STFT(frame_length, hop_length, window, win_length),
                                          STFTDecomposer()]

    def _plan(self, sample_rate):
        rt.require_card_geometry("AWAREDetector", self.frame_length, self.hop_length, self.win_length)
        return get_plan(self.frame_length, self.hop_length, self.window,
                        band_bins(sample_rate, self.frame_length, self.embedding_bands), win_length=self.win_length)

    def _centre(self) -> float:
        """What an undecided read-out value is: 0.5 behind a sigmoid, 0 otherwise."""
        return 0.5 if getattr(self.detection_net, "final_activation", "tanh") == "sigmoid" else 0.0

    def detect_batch(self, clips, sample_rate: int, sync_search=None, return_sync: bool = False):
        """list of 1-D float arrays (any lengths) -> device tensor [B, n_bits] of raw values.  sync_search (default: the
        detector's own, 0 = off): the number of views per clip of the offset search.  return_sync: (values, the chosen views'
        offsets in samples [B] int32, their confidence mean |value - centre| [B] float32) instead."""
        n = self.sync_search if sync_search is None else sync.check_sync_search(sync_search)
        plan = self._plan(sample_rate)
        det = self.detection_net.device_weights(plan)
        if n == 0:
            batch = rt.Batch([len(c) for c in clips])
            vals = rt.detect(plan, det, batch, batch.pack(clips))
            if not return_sync:
                return vals
            return vals, torch.zeros(len(clips), dtype=torch.int32, device=vals.device), (vals - self._centre()).abs().mean(dim=1)
        lengths = [len(c) for c in clips]
        vlen, voff = sync.sync_views(lengths, n)                  # ValueError for a clip too short, before any launch
        starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
        flat = torch.zeros(int(sum(lengths)), dtype=torch.float32, device=self.device)
        for c, o, m in zip(clips, starts, lengths):
            flat[int(o):int(o) + m] = torch.as_tensor(c, dtype=torch.float32)
        per = max(1, sync.SYNC_MAX_ROWS // n)                     # clips per aware_detect call
        outs = []
        for b0 in range(0, len(clips), per):
            b1 = min(len(clips), b0 + per)
            # the views of a clip share its samples: one batch with overlapping in_offsets, no copies
            views = rt.Batch(vlen[b0 * n:b1 * n], [int(starts[b]) + voff[b * n + j] for b in range(b0, b1) for j in range(n)])
            outs.append(rt.sync_select(rt.detect(plan, det, views, flat), n, self._centre()))
        vals = torch.cat([o[0] for o in outs])
        if not return_sync:
            return vals
        step = sync.SYNC_PERIOD // n
        return vals, torch.cat([o[1] for o in outs]) * step, torch.cat([o[2] for o in outs])

    def detect_device(self, audio: torch.Tensor, batch: "rt.Batch", sample_rate: int) -> torch.Tensor:
        plan = self._plan(sample_rate)
        return rt.detect(plan, self.detection_net.device_weights(plan), batch, audio)

    def detect(self, audio: np.ndarray, sample_rate: int, sync_search=None) -> np.ndarray:
        vals = self.detect_batch([np.asarray(audio, dtype=np.float32)], sample_rate, sync_search=sync_search)
        return vals[0].detach().cpu().numpy()
