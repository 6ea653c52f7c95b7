"""Batched embed -> attack -> detect driver: the loop of the reference's harness
(/root/reference/scripts/test.py:52-106) with every stage resident on the GPU.

One call processes a ragged batch of clips: optional 44.1 kHz -> 16 kHz polyphase front end
(scripts/test.py:60-63), embed (400 iterations per clip), the attack stage, detect, BER."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from . import runtime as rt
from .attacks import resample_poly_batch


@dataclass
class PipelineResult:
    bits: torch.Tensor                    # [B, n_bits] detected bits after the attack stage (device, int32)
    values: torch.Tensor                  # [B, n_bits] raw detector outputs
    bit_errors: torch.Tensor              # scalar tensor: number of wrong bits
    clean_bit_errors: torch.Tensor        # scalar tensor: wrong bits without any attack
    watermarked: "rt.Ragged" = None
    per_attack_errors: dict = field(default_factory=dict)
    seconds: float = 0.0                  # waveform-seconds processed (at the input rate)
    snr_db: torch.Tensor = None           # [B] float64: watermarked vs host clip at 16 kHz (report_snr=True)
    watermarked_out: "rt.Ragged" = None   # watermarked clips converted to `output_rate` (when requested)
    stoi: torch.Tensor = None             # [B] float64: STOI of the watermarked vs the host clip at 16 kHz (report_stoi=True)


class WatermarkPipeline:
    def __init__(self, embedder, detector, attacks=(), sample_rate: int = 16000, attack_mode: str = "chain"):
        if attack_mode not in ("chain", "each"):
            raise ValueError("attack_mode must be 'chain' or 'each'")
        self.embedder, self.detector = embedder, detector
        self.attacks = list(attacks)
        self.sample_rate = sample_rate
        self.attack_mode = attack_mode
        self._sessions = {}
        self._host16k = None

    def prepare(self, lengths_16k, input_rate: int | None = None):
        """One-time set-up for a batch geometry (lengths at the pipeline's 16 kHz): geometry tables,
        workspace, measured GEMM tile choice, hipGraph capture, resampler design.  Not part of a step."""
        key = tuple(int(n) for n in lengths_16k)
        if key not in self._sessions:
            b = self.embedder.make_batch(list(key), self.sample_rate)
            self._sessions[key] = (b, self.embedder.start_session(b, self.sample_rate))
        batch, sess = self._sessions[key]
        sess.iterate(0)                                    # records the graphs without running them
        dkey = ("det",) + tuple(batch.out_lengths)
        if dkey not in self._sessions:
            self._sessions[dkey] = self.detector.make_batch(batch.out_lengths, self.sample_rate)
        if input_rate and input_rate != self.sample_rate:
            from .attacks import _resample_filter
            g = int(np.gcd(self.sample_rate, input_rate))
            _resample_filter(self.sample_rate // g, input_rate // g, torch.device("cuda", torch.cuda.current_device()))
        return batch

    @staticmethod
    def _clip_max(x: "rt.Ragged") -> torch.Tensor:
        """signed per-clip maximum (service/embed.py:69)"""
        if len(set(x.lengths)) == 1:
            return x.data.view(x.B, -1).amax(dim=1)
        return torch.segment_reduce(x.data, "max", lengths=x.d_len.long())

    def _detect_bits(self, x: "rt.Ragged"):
        data = x.data if x.data.dtype == torch.float32 else x.data.float()
        key = ("det",) + tuple(x.lengths)
        if key not in self._sessions:
            self._sessions[key] = self.detector.make_batch(x.lengths, self.sample_rate)
        vals = self.detector.detect_device(data, self._sessions[key], self.sample_rate)
        return (vals > self.detector.threshold).to(torch.int32), vals

    def run(self, audio: "rt.Ragged", bits: torch.Tensor, input_rate: int | None = None, chains=None,
            chain_of_clip=None, report_snr: bool = False, output_rate: int | None = None,
            chains_by_kind=None, report_stoi: bool = False) -> PipelineResult:
        res = self._run(audio, bits, input_rate, chains, chain_of_clip, chains_by_kind)
        if report_snr:
            # imperceptibility metric of the reference (metrics/audio.py:68-89) on the device: watermarked clip
            # against the 16 kHz host clip over their common length
            res.snr_db = rt.snr_db(res.watermarked, self._host16k)
        if report_stoi:
            # the reference's third figure per file (scripts/test.py:41-92, metrics/audio.py:42-64), on the device
            res.stoi = rt.stoi(res.watermarked, self._host16k, self.sample_rate)
        if output_rate and output_rate != self.sample_rate:
            # back end of the 44.1 kHz flow (README.md:26-37 of the reference): polyphase 16 kHz -> output_rate
            res.watermarked_out = resample_poly_batch(res.watermarked, output_rate, self.sample_rate)
        self._host16k = None
        return res

    def _apply_chains_staged(self, wm: "rt.Ragged", kinds_of_clip, factory) -> "rt.Ragged":
        """Per-clip attack chains given as lists of attack KINDS (BASELINE config 5).  Stage s applies, for every
        kind, ONE batched launch sequence to the clips whose chain has that kind at position s (at most
        stages x kinds sub-batches however many distinct chains there are), so no workgroup branches on the attack
        kind and the detector then runs once over all clips."""
        cur = [wm.data[o:o + n] for o, n in zip(wm.offsets, wm.lengths)]
        cache = self._sessions.setdefault(("attacks",), {})
        depth = max((len(k) for k in kinds_of_clip), default=0)
        for s in range(depth):
            groups = {}
            for i, k in enumerate(kinds_of_clip):
                if s < len(k):
                    groups.setdefault(k[s], []).append(i)
            for kind in sorted(groups):
                members = groups[kind]
                if kind not in cache:
                    cache[kind] = factory(kind)
                parts = [cur[i] if cur[i].dtype == torch.float32 else cur[i].float() for i in members]
                sub = rt.Ragged(torch.cat(parts) if len(parts) > 1 else parts[0].contiguous(), [int(p.numel()) for p in parts])
                y = cache[kind].apply_batch(sub, self.sample_rate)
                for i, o, n in zip(members, y.offsets, y.lengths):
                    cur[i] = y.data[o:o + n]
        parts = [c if c.dtype == torch.float32 else c.float() for c in cur]
        return rt.Ragged(torch.cat(parts), [int(p.numel()) for p in parts])

    def _run(self, audio: "rt.Ragged", bits: torch.Tensor, input_rate: int | None = None, chains=None,
             chain_of_clip=None, chains_by_kind=None) -> PipelineResult:
        """audio: ragged device clips at `input_rate` (default: the pipeline's 16 kHz);
        bits: device int tensor [B, n_bits] of 0/1.
        chains / chain_of_clip (BASELINE config 5): `chains` is a list of attack lists and
        `chain_of_clip[b]` the index of the chain applied to clip b; clips are grouped by chain so that
        no workgroup ever branches on the attack kind."""
        input_rate = input_rate or self.sample_rate
        seconds = float(sum(audio.lengths)) / float(input_rate)
        x = audio
        if input_rate != self.sample_rate:
            x = resample_poly_batch(audio, self.sample_rate, input_rate)            # scripts/test.py:60-63
        self._host16k = x
        key = tuple(x.lengths)
        if key not in self._sessions:          # geometry tables + workspace are reused across steps
            b = self.embedder.make_batch(x.lengths, self.sample_rate)
            self._sessions[key] = (b, self.embedder.start_session(b, self.sample_rate))
        batch, sess = self._sessions[key]
        if getattr(self.embedder, "pattern_mode", "bits2bipolar") in ("bytes2bits", "bits"):
            target = bits.to(torch.float32)                                        # unipolar card: the bits themselves
        else:
            target = (2 * bits - 1).to(torch.float32)                              # PatternEncoder bits2bipolar
        out, _ = self.embedder.embed_device(x.data, batch, self.sample_rate, target, self._clip_max(x), session=sess)
        wm = rt.Ragged(out, batch.out_lengths)
        clean_bits, clean_vals = self._detect_bits(wm)
        clean_err = (clean_bits != bits).sum()
        per = {}
        if chains_by_kind is not None:
            kinds_of_clip, factory = chains_by_kind
            y = self._apply_chains_staged(wm, kinds_of_clip, factory)
            det_bits, vals = self._detect_bits(y)
            err = (det_bits != bits).sum()
            return PipelineResult(det_bits, vals, err, clean_err, wm, per, seconds)
        if chains is not None:
            det_bits = torch.empty_like(clean_bits)
            vals = torch.empty_like(clean_vals)
            for cid, chain in enumerate(chains):
                members = [i for i, c in enumerate(chain_of_clip) if c == cid]
                if not members:
                    continue
                y = wm.select(members)
                for a in chain:
                    if y.data.dtype != torch.float32:
                        y = rt.Ragged(y.data.float(), y.lengths)
                    y = a.apply_batch(y, self.sample_rate)
                gb, gv = self._detect_bits(y)
                idx = torch.tensor(members, device=bits.device)
                det_bits[idx] = gb
                vals[idx] = gv
                per["+".join(a.name for a in chain) or "none"] = (gb != bits[idx]).sum()
            err = (det_bits != bits).sum()
            return PipelineResult(det_bits, vals, err, clean_err, wm, per, seconds)
        if not self.attacks:
            return PipelineResult(clean_bits, clean_vals, clean_err, clean_err, wm, per, seconds)
        if self.attack_mode == "chain":
            y = wm
            for a in self.attacks:
                if y.data.dtype != torch.float32:
                    y = rt.Ragged(y.data.float(), y.lengths)
                y = a.apply_batch(y, self.sample_rate)
            det_bits, vals = self._detect_bits(y)
            err = (det_bits != bits).sum()
            per["+".join(a.name for a in self.attacks)] = err
            return PipelineResult(det_bits, vals, err, clean_err, wm, per, seconds)
        total = torch.zeros((), dtype=torch.int64, device=bits.device)
        det_bits, vals = clean_bits, clean_vals
        for a in self.attacks:
            y = a.apply_batch(wm, self.sample_rate)
            det_bits, vals = self._detect_bits(y)
            e = (det_bits != bits).sum()
            per[a.name] = e
            total = total + e
        return PipelineResult(det_bits, vals, total, clean_err, wm, per, seconds)


def synthetic_clips(n_clips: int, seconds: float, rate: int, first_seed: int = 0, device="cuda"):
    """Synthetic workload of BASELINE.json: sigma = 0.1 Gaussian clips, 20 random bits per clip,
    generated on the device from the clip's global index (so every rank draws its own shard)."""
    n = int(round(seconds * rate))
    audio = torch.empty((n_clips, n), dtype=torch.float32, device=device)
    bits = torch.empty((n_clips, 20), dtype=torch.int32, device=device)
    for i in range(n_clips):
        g = torch.Generator(device=device).manual_seed(1_000_003 * (first_seed + i) + 17)
        audio[i] = 0.1 * torch.randn(n, generator=g, device=device)
        bits[i] = torch.randint(0, 2, (20,), generator=g, device=device, dtype=torch.int32)
    return rt.Ragged(audio.reshape(-1), [n] * n_clips), bits


def synthetic_ragged_clips(seconds, rate: int, seeds=None, device="cuda"):
    """Mixed-length variant (BASELINE config 5): clip i lasts seconds[i] s; seeded by seeds[i] (default: its index)."""
    lengths = [int(round(float(sec) * rate)) for sec in seconds]
    seeds = list(range(len(lengths))) if seeds is None else list(seeds)
    audio = torch.empty(sum(lengths), dtype=torch.float32, device=device)
    bits = torch.empty((len(lengths), 20), dtype=torch.int32, device=device)
    o = 0
    for i, (n, sd) in enumerate(zip(lengths, seeds)):
        g = torch.Generator(device=device).manual_seed(1_000_003 * int(sd) + 17)
        audio[o:o + n] = 0.1 * torch.randn(n, generator=g, device=device)
        bits[i] = torch.randint(0, 2, (20,), generator=g, device=device, dtype=torch.int32)
        o += n
    return rt.Ragged(audio, lengths), bits


def run_folder(folder, embedder, detector, attacks=(), watermark_length: int = 20, seed: int | None = None,
               pattern: str = "*.wav") -> dict:
    """The reference's harness loop over a folder of audio files (`scripts/test.py:52-106`): load mono at the native
    rate, resample to 16 kHz when needed, embed a random watermark, detect, then apply every attack on its own and detect
    again.  Returns `{"files": [...], "orig": [BER % per file], attack.name: [BER % per file], ..., "snr_db": [...],
    "stoi": [...]}` -- the `rec` dictionary of the reference (BER in percent, `metrics/audio.py:8-17`) plus the SNR and the
    STOI of each watermarked file.  The reference appends a STOI score only when it is above 0.1 (to keep silent files out
    of its mean); here `rec["stoi"]` stays aligned with `rec["files"]`, one value per file, and the caller filters.
    Files are WAV (`aware_amd.utils.audio.io`); clips of one native rate are embedded as one ragged batch; a file the
    reference would refuse (too short for the STFT) is skipped with its error recorded under "skipped"."""
    from pathlib import Path
    from .utils.audio import io
    rng = np.random.default_rng(seed)
    paths = sorted(Path(folder).glob(pattern))
    rec = {"files": [], "orig": [], "snr_db": [], "stoi": [], "skipped": []}
    by_rate = {}
    for p in paths:
        try:
            x, sr = io.load(str(p), sr=None, mono=True)
        except ValueError as e:
            rec["skipped"].append((p.name, str(e)))
            continue
        if -(-len(x) * 16000 // sr) <= 512:      # polyphase output length ceil(n * up / down); torch.stft's reflect padding needs > n_fft / 2
            rec["skipped"].append((p.name, "clip too short"))
            continue
        by_rate.setdefault(sr, []).append((p.name, x))
    for sr, items in sorted(by_rate.items()):
        names = [n for n, _ in items]
        audio = rt.Ragged.from_list([x for _, x in items])
        bits = torch.as_tensor(rng.integers(0, 2, size=(len(items), watermark_length)), dtype=torch.int32, device="cuda")
        pipe = WatermarkPipeline(embedder, detector, attacks=[])
        res = pipe.run(audio, bits, input_rate=sr, report_snr=True, report_stoi=True)
        wm_bits, _ = pipe._detect_bits(res.watermarked)
        rec["files"] += names
        rec["orig"] += (100.0 * (wm_bits != bits).float().mean(dim=1)).cpu().tolist()
        rec["snr_db"] += res.snr_db.cpu().tolist()
        rec["stoi"] += res.stoi.cpu().tolist()
        for a in attacks:
            attacked = a.apply_batch(res.watermarked, 16000)
            a_bits, _ = pipe._detect_bits(attacked)
            rec.setdefault(a.name, [])
            rec[a.name] += (100.0 * (a_bits != bits).float().mean(dim=1)).cpu().tolist()
    return rec
