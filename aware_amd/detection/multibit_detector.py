"""AWAREDetector.detect on the HIP path.

Reference: src/AWARE/detection/multibit_detector.py:9-42 -- normalise, STFT, magnitude, zero the
bins outside the embedding band, network forward.  Batched entry point: detect_batch.  EXTENSION: sync_search = n reads n views of every clip, 512 / n samples
apart, and keeps the most confident one (detection/sync.py); off by default.  EXTENSION: speed_search reads every clip at
candidate playback speeds as well (same module); off by default.  EXTENSION: shift_search reads every clip at candidate
frequency shifts (same module); off by default, and not together with speed_search.  EXTENSION: scan
reads a long file in windows and returns the marked spans with one payload each (same module); off
unless called.  EXTENSION: payload_code names the channel code of the payload (utils/watermark/fec.py): decode_messages runs the Viterbi decoder over rows
of values, and scan() adds the decoded message to every span; absent = no code."""
from __future__ import annotations

import numpy as np
import torch

from ..interfaces import BaseDetector
from ..utils.audio import STFT, STFTDecomposer, WaveformNormalizer, band_bins, get_plan
from ..utils.watermark import fec
from .. import runtime as rt
from . import sync


class AWAREDetector(BaseDetector):
    def __init__(self, model, threshold: float = 0.0, frame_length: int = 1024, hop_length: int = 256,
                 window: str = "hann", win_length: int = 1024, pattern_mode: str = "bits2bipolar",
                 embedding_bands=(500, 4000), sync_search: int = 0, speed_search=None, scan=None, payload_code=None,
                 general_geometry: bool = False, shift_search=None):
        """general_geometry (EXTENSION): detect at any frame_length in runtime.GENERAL_NFFT, any
        hop_length and win_length in 1..frame_length, on the general route; off: the card geometry only.  With it sync_search,
        speed_search, shift_search and scan raise NotImplementedError (their offsets assume the card's 512-sample pooling period).
        The same four refuse a detection net whose initial pool is not (2, 2) (key initial_pools), here
        and per call: its read-out period is 256 * initial_pool_stride samples."""
        self.general_geometry = bool(general_geometry)
        rt.require_card_geometry("AWAREDetector", frame_length, hop_length, win_length, self.general_geometry, window)
        self.sync_search = sync.check_sync_search(sync_search)
        self.speed_search = sync.check_speed_search(speed_search)
        if self.general_geometry and self.sync_search:
            rt.refuse_general_geometry("sync_search")
        if self.general_geometry and self.speed_search is not None:
            rt.refuse_general_geometry("speed_search")
        self.shift_search = sync.check_shift_search(shift_search)
        if self.general_geometry and self.shift_search is not None:
            rt.refuse_general_geometry("shift_search")
        if self.speed_search is not None and self.shift_search is not None:
            raise ValueError("AWAREDetector: speed_search and shift_search are both on; the product of the two grids is not served")
        self.detection_net = model
        self._refuse_pool(self.sync_search, self.speed_search, self.shift_search)
        if scan is not None:
            self._refuse_pool(scan=True)
        if self.general_geometry and model is not None and getattr(model, "n_fft", frame_length) != frame_length:
            raise ValueError(f"AWAREDetector: the detection net's n_fft = {model.n_fft} but frame_length = {frame_length}; "
                             f"with general_geometry the detector's mel bank follows the STFT")
        self.scan_defaults = sync.check_scan_card(scan)           # what scan() uses where its arguments are None
        self.scan_rows_per_call = sync.SYNC_MAX_ROWS              # rows per aware_detect call of scan()
        self.payload_code = fec.check_payload_code(payload_code)  # the channel code of service.detect_message and scan()
        if self.payload_code:
            fec.capacity(model.output_length, **self.payload_code)            # ValueError where no message bit is left
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
        rt.require_card_geometry("AWAREDetector", self.frame_length, self.hop_length, self.win_length, self.general_geometry,
                                 self.window)
        return get_plan(self.frame_length, self.hop_length, self.window,
                        band_bins(sample_rate, self.frame_length, self.embedding_bands), win_length=self.win_length,
                        general=self.general_geometry)

    def make_batch(self, lengths, sample_rate: int) -> "rt.Batch":
        """The batch geometry of this detector's plan for clips of `lengths` samples (with general_geometry: ValueError
        naming a clip of n_fft/2 samples or fewer)."""
        self._check_tap_clips(lengths)
        if not self.general_geometry:
            return rt.Batch(list(lengths))
        rt.check_general_clips("AWAREDetector", self.frame_length, self.hop_length, self.win_length, self.window, lengths,
                               embed=False)
        return rt.Batch(list(lengths), plan=self._plan(sample_rate))

    def _refuse_pool(self, n: int = 0, speed=None, shift=None, scan: bool = False):
        """NotImplementedError where a search is on and the net's initial pool is not (2, 2)."""
        pool = tuple(getattr(self.detection_net, "pool", (2, 2)))
        if pool == (2, 2):
            return
        for on, what in ((n, "sync_search"), (speed is not None, "speed_search"), (shift is not None, "shift_search"),
                         (scan, "scan")):
            if on:
                rt.refuse_initial_pool(what, pool)

    def _check_tap_clips(self, lengths):
        """A net of temporal convolutions or with another initial pool: ValueError naming the first clip that the pool or some
        block leaves without a row."""
        check = getattr(self.detection_net, "check_clip_frames", None)
        if check is not None:
            check("AWAREDetector", [1 + int(n) // self.hop_length for n in lengths])

    def _centre(self) -> float:
        """What an undecided read-out value is: 0.5 behind a sigmoid, 0 otherwise."""
        return 0.5 if getattr(self.detection_net, "final_activation", "tanh") == "sigmoid" else 0.0

    def decode_messages(self, values) -> list:
        """values [R, L] (device tensor or numpy) of coded frames -> per row {"message" int32 [k], "bytes" (the first k // 8
        bytes), "valid", "corrected", "metric"}: one aware_viterbi_decode over all rows.  ValueError without a payload_code."""
        code = self.payload_code
        if not code:
            raise ValueError("decode_messages: this detector has no payload_code")
        v = torch.as_tensor(values, dtype=torch.float32).to(self.device)
        k = fec.capacity(v.shape[-1], **code)
        out = {name: t.cpu().numpy() for name, t in rt.viterbi_decode(v, self._centre(), code["rate"], code["crc"]).items()}
        bits = fec.unpack_bits(out["bits"], k)
        return [{"message": bits[r], "bytes": fec.message_bytes(bits[r]), "valid": bool(out["valid"][r]),
                 "corrected": int(out["corrected"][r]), "metric": float(out["metric"][r])} for r in range(len(bits))]

    def detect_batch(self, clips, sample_rate: int, sync_search=None, return_sync: bool = False, speed_search=None,
                     return_speed: bool = False):
        """list of 1-D float arrays (any lengths) -> device tensor [B, n_bits] of raw values.  sync_search (default: the
        detector's own, 0 = off): the number of views per clip of the offset search.  return_sync: (values, the chosen views'
        offsets in samples [B] int32, their confidence mean |value - centre| [B] float32) instead.  speed_search (default: the
        detector's own, None = off): max_percent or {"max_percent", "step_percent"} of the speed search.  return_speed:
        (values, offsets [B] int32, the chosen views' speed offsets m [B] int32 -- the clip was played at sync.speed_of(m) --
        confidence [B] float32) instead.  A detector with shift_search on reads through its shift search here as well (m is
        then 0); detect_batch_shift takes that key per call and returns the chosen shifts."""
        return self._detect_any(clips, sample_rate, sync_search, return_sync, speed_search, return_speed, None, False)

    def detect_batch_shift(self, clips, sample_rate: int, shift_search=None, sync_search=None, return_shift: bool = False):
        """detect_batch through the shift search.  shift_search (default: the detector's own, None =
        off): max_hz or {"max_hz", "step_hz"}.  return_shift: (values, offsets [B] int32, the chosen views' shifts d [B] int32
        in units of sample_rate / 2^20 Hz -- the clip carried a shift of sync.shift_of(d, sample_rate) Hz -- confidence [B]
        float32) instead of the values.  ValueError, before any launch: the search together with the detector's speed_search
        (the product of the two grids is not served), max_hz above sample_rate / 16, a clip of 512 samples or fewer."""
        return self._detect_any(clips, sample_rate, sync_search, False, None, False, shift_search, return_shift)

    def _detect_any(self, clips, sample_rate, sync_search, return_sync, speed_search, return_speed, shift_search, return_shift):
        n = self.sync_search if sync_search is None else sync.check_sync_search(sync_search)
        speed = self.speed_search if speed_search is None else sync.check_speed_search(speed_search)
        shift = self.shift_search if shift_search is None else sync.check_shift_search(shift_search)
        if self.general_geometry and n:
            rt.refuse_general_geometry("sync_search")
        if self.general_geometry and speed is not None:
            rt.refuse_general_geometry("speed_search")
        if self.general_geometry and shift is not None:
            rt.refuse_general_geometry("shift_search")
        if speed is not None and shift is not None:
            raise ValueError("AWAREDetector: speed_search and shift_search are both on; the product of the two grids is not served")
        self._refuse_pool(n, speed, shift)
        if self.general_geometry:                                 # ValueError naming the clip, before any plan or launch
            rt.check_general_clips("AWAREDetector", self.frame_length, self.hop_length, self.win_length, self.window,
                                   [len(c) for c in clips], embed=False)
        self._check_tap_clips([len(c) for c in clips])
        four = return_speed or return_shift
        if speed is None and shift is None:
            out = self._detect_sync(clips, sample_rate, n, return_sync or four)
            if four:
                return out[0], out[1], torch.zeros(len(clips), dtype=torch.int32, device=out[0].device), out[2]
            return out
        if shift is not None:
            vals, offsets, grid, conf = self._detect_shift(clips, sample_rate, n, shift)
        else:
            vals, offsets, grid, conf = self._detect_speed(clips, sample_rate, n, speed)
        if four:                                                  # return_speed of a shift search: m = 0, the speed is the clip's own
            return vals, offsets, grid if return_shift == (shift is not None) else torch.zeros_like(grid), conf
        return (vals, offsets, conf) if return_sync else vals

    def _detect_sync(self, clips, sample_rate: int, n: int, return_sync: bool):
        plan = self._plan(sample_rate)
        det = self.detection_net.device_weights(plan)
        if n == 0:
            batch = self.make_batch([len(c) for c in clips], sample_rate)
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

    def _detect_speed(self, clips, sample_rate: int, n: int, speed: dict):
        """(values, offsets, m, confidence) of the speed search `speed`, times the offset search where n > 0: every clip at
        every speed offset in one aware_speed_views launch per chunk, one aware_detect over all the views (with n > 0 over the
        n overlapping windows into each), then aware_sync_select over the sync views and once more over the speed views."""
        ms = sync.speed_offsets(speed)
        vlen = sync.speed_views([len(c) for c in clips], speed, n)             # ValueError for a clip too short or too long, before any launch
        return self._detect_views(clips, sample_rate, n, ms, vlen, lambda sub: rt.speed_views(sub, ms), sync.SPEED_MAX_SAMPLES,
                                  "speed_search")

    def _detect_shift(self, clips, sample_rate: int, n: int, shift: dict):
        """(values, offsets, d, confidence) of the shift search `shift`, times the offset search where n > 0: every clip at
        every candidate shift in one aware_shift_views launch per chunk, then as _detect_speed."""
        ds = sync.shift_offsets(shift, sample_rate)               # ValueError for max_hz above sample_rate / 16
        vlen = sync.shift_views([len(c) for c in clips], shift, sample_rate, n)            # ValueError for a clip too short or too long
        return self._detect_views(clips, sample_rate, n, ds, vlen, lambda sub: rt.shift_views(sub, ds), sync.SHIFT_MAX_SAMPLES,
                                  "shift_search")

    def _detect_views(self, clips, sample_rate: int, n: int, grid, vlen, views, max_samples: int, what: str):
        """What the speed and the shift search share: `views(sub)` writes the len(grid) views of every clip of a chunk (their
        lengths vlen, clip-major), one aware_detect reads all rows (with n > 0 the n overlapping windows into each view), and
        aware_sync_select picks over the sync views and then over the grid -> (values, offsets, grid value, confidence)."""
        ns, nw = len(grid), max(n, 1)
        if ns * nw > sync.SYNC_MAX_ROWS:
            raise ValueError(f"{what} with sync_search = {n}: {ns} x {nw} views per clip; at most {sync.SYNC_MAX_ROWS}")
        plan = self._plan(sample_rate)
        det = self.detection_net.device_weights(plan)
        x = rt.Ragged.from_list([np.asarray(c, dtype=np.float32) for c in clips])
        offs = sync.sync_offsets(n)
        centre = self._centre()
        md = torch.tensor(grid, dtype=torch.int32, device=x.data.device)
        # chunks of whole clips: at most SYNC_MAX_ROWS rows per aware_detect call and 2^30 view samples per buffer
        padded = [sum((v + 3) // 4 * 4 for v in vlen[b * ns:(b + 1) * ns]) for b in range(len(clips))]
        chunks, b0, size = [], 0, 0
        for b in range(len(clips)):
            if b > b0 and ((b - b0 + 1) * ns * nw > sync.SYNC_MAX_ROWS or size + padded[b] > max_samples):
                chunks.append((b0, b))
                b0, size = b, 0
            size += padded[b]
        chunks.append((b0, len(clips)))
        outs = []
        for b0, b1 in chunks:
            sub = x if (b0, b1) == (0, x.B) else rt.Ragged(x.data[x.offsets[b0]:x.offsets[b1 - 1] + x.lengths[b1 - 1]], x.lengths[b0:b1])
            flat, sl, so = views(sub)
            rows = rt.Batch([v - e for v in sl for e in offs], [o + e for o in so for e in offs])
            vals = rt.detect(plan, det, rows, flat)               # [(b1 - b0) * ns * nw, n_bits]
            if n:
                vals, isync, _ = rt.sync_select(vals, n, centre)  # round one: the sync views of every (clip, grid view)
            best, igrid, conf = rt.sync_select(vals, ns, centre)  # round two: the grid views of every clip
            if n:
                chosen = isync.view(b1 - b0, ns).gather(1, igrid.long()[:, None])[:, 0] * (sync.SYNC_PERIOD // n)
            else:
                chosen = torch.zeros(b1 - b0, dtype=torch.int32, device=best.device)
            outs.append((best, chosen.to(torch.int32), md[igrid.long()], conf))
        return tuple(torch.cat([o[i] for o in outs]) for i in range(4))

    def scan(self, clips, sample_rate: int, window_seconds=None, hop_samples=None, sync_search=None, min_confidence=None,
             max_flip=None, max_segments=None, return_profile: bool = False):
        """list of 1-D float arrays (files of any lengths) -> per file the list of its marked spans, in order.  Every file is
        read in windows of window_seconds (default 1.0) every hop_samples (4096), each at the sync_search views of the offset
        search (None: the detector's own, or 8 where that is off; an explicit 0 or 1: one view per window, no offsets); a
        window is marked where the confidence mean |value - centre| of its best view reaches min_confidence (0.06; at 0 or
        below, windows of confidence 0 are marked and a span of such windows alone has values 0 / 0), and marked neighbours
        whose bits differ in at most max_flip (n_bits // 4) places form one span; the first max_segments (16) spans of a file are returned.  The four
        defaults are the detector's scan_defaults (the card key `scan`).  A span is a dict of `start` and `end` (samples: the
        first window's start, the last window's start plus the window length), `peak` (samples: the most confident window's
        start plus its view's offset), `confidence` (that window's), `values` [n_bits] float32 (the confidence-weighted mean of
        the span's windows: decode these) and `windows` (first, last: indices into the profile); with a payload_code on the
        detector also `message`, `valid` and `corrected` of decode_messages (valid informs; it does not filter).  return_profile: (spans,
        profiles) instead, a profile per file being a dict of `starts` (the window starts), `length` (samples per window),
        `win_conf`, `win_view` and `win_values` (numpy, per window: the best view's confidence, index and row) and `n_segments` (the true span count, which max_segments may have cut).
        ValueError, before any launch: a parameter check_scan refuses, a file too short (by its index), speed_search or
        shift_search on."""
        if self.general_geometry:
            rt.refuse_general_geometry("scan")
        self._refuse_pool(scan=True)
        if self.speed_search is not None:
            raise ValueError("scan: speed_search is on for this detector; scanning at candidate speeds is not supported")
        if self.shift_search is not None:
            raise ValueError("scan: shift_search is on for this detector; scanning at candidate frequency shifts is not supported")
        d = self.scan_defaults
        par = sync.check_scan(d["window_seconds"] if window_seconds is None else window_seconds,
                              d["hop_samples"] if hop_samples is None else hop_samples,
                              d["min_confidence"] if min_confidence is None else min_confidence,
                              d["max_segments"] if max_segments is None else max_segments, max_flip, sample_rate)
        n = (self.sync_search or sync.SCAN_SYNC) if sync_search is None else (sync.check_sync_search(sync_search) or 1)
        offs = sync.sync_offsets(n)
        lengths = [len(c) for c in clips]
        if not lengths:
            return ([], []) if return_profile else []
        geometry = [sync.scan_windows(m, par["window"], par["hop_samples"], n, index=b) for b, m in enumerate(lengths)]
        plan = self._plan(sample_rate)
        det = self.detection_net.device_weights(plan)
        if det.n_bits > sync.SCAN_MAX_BITS:
            raise ValueError(f"scan: payloads of {det.n_bits} bits; at most {sync.SCAN_MAX_BITS}")
        flip = det.n_bits // 4 if par["max_flip"] is None else par["max_flip"]
        base = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
        flat = torch.zeros(int(sum(lengths)), dtype=torch.float32, device=self.device)
        for c, o, m in zip(clips, base, lengths):
            flat[int(o):int(o) + m] = torch.as_tensor(c, dtype=torch.float32)
        # the views of all windows share the files' samples: batches with overlapping in_offsets, no copies
        row_off = [int(o) + s + e for o, (starts, _) in zip(base, geometry) for s in starts for e in offs]
        row_len = [length for starts, length in geometry for _ in starts for _ in offs]
        win_off = np.concatenate([[0], np.cumsum([len(starts) for starts, _ in geometry])]).astype(np.int64).tolist()
        per = max(1, int(self.scan_rows_per_call))
        vals = torch.cat([rt.detect(plan, det, rt.Batch(row_len[r:r + per], row_off[r:r + per]), flat)
                          for r in range(0, len(row_off), per)])
        centre = self._centre()
        win_values, win_view, win_conf, win_bits = rt.scan_select(vals, win_off, n, centre)
        seg = rt.scan_segments(win_conf, win_view, win_values, win_bits, win_off, centre, par["min_confidence"], flip,
                               par["max_segments"])
        host = {k: v.cpu().numpy() for k, v in seg.items()}
        conf_h, view_h, rows_h = win_conf.cpu().numpy(), win_view.cpu().numpy(), win_values.cpu().numpy()
        spans, profiles = [], []
        for b, (starts, length) in enumerate(geometry):
            found = []
            for r in range(min(int(host["n_seg"][b]), par["max_segments"])):
                first, last, peak = (int(host[k][b, r]) for k in ("first", "last", "peak"))
                found.append({"start": starts[first], "end": starts[last] + length,
                              "peak": starts[peak] + offs[int(host["view"][b, r])], "confidence": float(host["confidence"][b, r]),
                              "values": host["values"][b, r].copy(), "windows": (first, last)})
            spans.append(found)
            profiles.append({"starts": list(starts), "length": length, "win_conf": conf_h[win_off[b]:win_off[b + 1]].copy(),
                             "win_view": view_h[win_off[b]:win_off[b + 1]].copy(),
                             "win_values": rows_h[win_off[b]:win_off[b + 1]].copy(), "n_segments": int(host["n_seg"][b])})
        every = [s for found in spans for s in found]
        if self.payload_code and every:                           # one decode over all spans of all files
            for s, m in zip(every, self.decode_messages(np.stack([s["values"] for s in every]))):
                s.update(message=m["message"], valid=m["valid"], corrected=m["corrected"])
        return (spans, profiles) if return_profile else spans

    def detect_device(self, audio: torch.Tensor, batch: "rt.Batch", sample_rate: int) -> torch.Tensor:
        plan = self._plan(sample_rate)
        return rt.detect(plan, self.detection_net.device_weights(plan), batch, audio)

    def detect(self, audio: np.ndarray, sample_rate: int, sync_search=None, speed_search=None) -> np.ndarray:
        vals = self.detect_batch([np.asarray(audio, dtype=np.float32)], sample_rate, sync_search=sync_search,
                                 speed_search=speed_search)
        return vals[0].detach().cpu().numpy()
