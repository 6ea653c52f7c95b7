"""Attack stage between embed and detect, on the GPU.

Reference: /root/reference/scripts/attacks.py -- an `Attack` ABC with `.apply(audio, sr)` and a
`.name`, instantiated into a hand-built list by the harness (scripts/test.py:15-18).  The same
classes, constructor arguments and names are kept; each also has `apply_batch(Ragged, sr)` that
runs a whole ragged batch through libaware_hip.so without leaving HBM.  A name -> class registry
(`ATTACKS`, `make_attack`) replaces the hand-built list so that attack chains can be sampled by
name per clip (BASELINE.json config 5).

Random draws stay on the host with the reference's generators (`random.uniform`,
`np.random.randint`), one draw per clip in batch order.

Filter DESIGN (Butterworth coefficients, Kaiser FIR) is done once on the host with scipy.signal,
exactly the calls the reference makes; the filtering itself runs in the HIP kernels.

Out of scope here (external binaries, no offline oracle): MP3Compression (ffmpeg),
TimeStretch / PitchShift (rubberband) -- see DESIGN.md."""
from __future__ import annotations

import random
from abc import ABC, abstractmethod

import numpy as np
import torch

from . import runtime as rt

ATTACKS = {}


def register(cls):
    ATTACKS[cls.__name__] = cls
    return cls


def make_attack(kind: str, **kwargs) -> "Attack":
    if kind not in ATTACKS:
        raise ValueError(f"Unknown attack: {kind}. Available: {sorted(ATTACKS)}")
    return ATTACKS[kind](**kwargs)


class Attack(ABC):
    """scripts/attacks.py:16-30"""
    name = "attack"

    @abstractmethod
    def apply_batch(self, x: "rt.Ragged", sr: int) -> "rt.Ragged":
        ...

    def apply(self, audio, sr):
        out = self.apply_batch(rt.Ragged.from_list([np.asarray(audio, dtype=np.float32)]), sr)
        return out.to_list()[0]


@register
class PCMBitDepthConversion(Attack):
    """:33-70"""

    def __init__(self, pcm=16):
        self.pcm = pcm
        self.name = f"pcm_{pcm}"

    def apply_batch(self, x, sr):
        return rt.pcm_quantize(x, self.pcm)


_FIR_CACHE = {}


def _resample_filter(up, down, device):
    """scipy.signal.resample_poly's default design: firwin(20*max+1, 1/max, ('kaiser', 5.0)),
    cast to float32 (the input dtype) and scaled by `up` (scipy/_signaltools.py resample_poly)."""
    key = (up, down, str(device))
    if key not in _FIR_CACHE:
        from scipy.signal import firwin
        mx = max(up, down)
        half = 10 * mx
        h = firwin(2 * half + 1, 1.0 / mx, window=("kaiser", 5.0)).astype(np.float32)
        h *= up
        _FIR_CACHE[key] = (torch.from_numpy(h).to(device), half)
    return _FIR_CACHE[key]


def resample_poly_batch(x: "rt.Ragged", up: int, down: int) -> "rt.Ragged":
    g = int(np.gcd(up, down))
    up, down = up // g, down // g
    h, half = _resample_filter(up, down, x.data.device)
    return rt.upfirdn(x, h, up, down, half)


@register
class Resample(Attack):
    """:256-294.  sr // target_sr > 1: decimate without anti-alias filter + np.interp back (float64, :275-288);
    otherwise (the harness's sr == target == 16 kHz) the polyphase 441/160 round trip (:290-293)."""

    def __init__(self, target_sr=16000):
        self.target_sr = target_sr
        self.name = f"resample_{target_sr}"

    def apply_batch(self, x, sr):
        if sr // self.target_sr > 1:
            return rt.decimate_interp(x, sr // self.target_sr)
        return resample_poly_batch(resample_poly_batch(x, 441, 160), 160, 441)


def _butter(order, wn, btype):
    from scipy.signal import butter
    return butter(order, wn, btype=btype, analog=False)


class _LFilterAttack(Attack):
    btype = None

    def apply_batch(self, x, sr):
        b, a = _butter(self.order, self.cut_off / (0.5 * sr), self.btype)
        return rt.iir(x, np.tile(b, (x.B, 1)), np.tile(a, (x.B, 1)), out_f64=True)

    def apply(self, audio, sr):
        # the reference's lfilter returns float64 (:414, :452)
        out = self.apply_batch(rt.Ragged.from_list([np.asarray(audio, dtype=np.float32)]), sr)
        return out.to_list()[0]


@register
class LowPassFilter(_LFilterAttack):
    """:388-423"""
    btype = "low"

    def __init__(self, cut_off=4000.0, order=6):
        self.order, self.cut_off, self.name = order, cut_off, "low_pass"


@register
class HighPassFilter(_LFilterAttack):
    """:426-455"""
    btype = "highpass"

    def __init__(self, cut_off=500.0, order=4):
        self.order, self.cut_off, self.name = order, cut_off, "high_pass"


@register
class RandomBandstop(Attack):
    """:298-356 -- one random stop band per clip, zero-phase filtfilt in float64."""

    def __init__(self, band_width=200.0, min_freq=300.0, max_freq=4000.0, order=4):
        self.band_width, self.min_freq, self.max_freq, self.order = float(band_width), float(min_freq), float(max_freq), int(order)
        self.name = f"bandstop_{int(band_width)}Hz"

    def apply_batch(self, x, sr, f_low=None):
        from scipy.signal import lfilter_zi
        nyq = sr / 2.0
        bs, as_, zs = [], [], []
        for i in range(x.B):
            fl = random.uniform(self.min_freq, self.max_freq - self.band_width) if f_low is None else f_low[i]
            b, a = _butter(self.order, [fl / nyq, (fl + self.band_width) / nyq], "bandstop")
            bs.append(b), as_.append(a), zs.append(lfilter_zi(b, a))
        return rt.iir(x, np.stack(bs), np.stack(as_), np.stack(zs), filtfilt=True, out_f64=False)


@register
class DeleteSamples(Attack):
    """:151-178"""

    def __init__(self, percentage):
        self.percentage = percentage
        self.name = f"delete_{percentage}"

    def apply_batch(self, x, sr, starts=None):
        cuts = [int(self.percentage * n) for n in x.lengths]
        if starts is None:
            starts = [int(np.random.randint(0, n - k)) for n, k in zip(x.lengths, cuts)]
        return rt.segment_cut(x, starts, cuts, zero_fill=False)


@register
class Cropout(Attack):
    """:181-205 -- drops the first percentage*sr samples."""

    def __init__(self, percentage):
        self.percentage = percentage
        self.name = f"cropout_{percentage}"

    def apply_batch(self, x, sr):
        k = int(self.percentage * sr)
        return rt.segment_cut(x, [0] * x.B, [k] * x.B, zero_fill=False)


@register
class SampleSupression(Attack):
    """:359-385 (spelling as in the reference)"""

    def __init__(self, percentage):
        self.percentage = percentage
        self.name = f"sample_supression_{percentage}"

    def apply_batch(self, x, sr, starts=None):
        k = int(self.percentage * sr)
        if starts is None:
            starts = [int(np.random.randint(0, n - k)) for n in x.lengths]
        return rt.segment_cut(x, starts, [k] * x.B, zero_fill=True)


@register
class GaussianNoise(Attack):
    """EXTENSION (not in the reference; BASELINE.json north_star / config 3): additive white
    Gaussian noise at `snr_db`, Philox-4x32-10 keyed by the clip's seed.  Specified by
    oracle/aware_oracle.py::gaussian_noise_attack -- parity unpinned."""

    def __init__(self, snr_db=20.0, seed=0):
        self.snr_db, self.seed = float(snr_db), int(seed)
        self.name = f"gaussian_{int(snr_db)}dB"

    def apply_batch(self, x, sr, seeds=None):
        if seeds is None:
            seeds = [self.seed + i for i in range(x.B)]
        return rt.gaussian_noise(x, self.snr_db, seeds)


@register
class Reverberation(Attack):
    """EXTENSION (not in the reference, parity unpinned): a synthetic room response -- an exponentially decaying Gaussian
    tail of int(rt60 * sr) taps, 60 dB down at its end, behind a direct path drr_db above the tail's energy -- convolved with
    the clip, causal, truncated to the clip's length, not normalised.  Clip i draws the response of seed + i that
    embedding.loop_attacks.reverb_ir specifies at step 0, entry 0: what a {"kind": "reverberation", "rt60": rt60} entry of
    the embed loop applies at its first step."""

    def __init__(self, rt60=0.3, drr_db=-3.0, seed=0):
        self.rt60, self.drr_db, self.seed = float(rt60), float(drr_db), int(seed)
        self.name = f"reverb_{rt60}"

    def apply_batch(self, x, sr, seeds=None):
        if seeds is None:
            seeds = [self.seed + i for i in range(x.B)]
        n = int(self.rt60 * sr)
        h, nh = rt.reverb_ir(seeds, 0, 0, n, n, self.drr_db)
        return rt.convolve(x, h, nh)


@register
class GainEnvelope(Attack):
    """EXTENSION (not in the reference, parity unpinned): a gain that moves over time, piecewise linear between random
    breakpoints int(period * sr) samples apart, each breakpoint's gain uniform in [floor, 1].  Clip i draws the envelope of
    seed + i that embedding.loop_attacks.gain_envelope specifies at step 0, entry 0: what a {"kind": "gain_envelope",
    "period": period, "floor": floor} entry of the embed loop applies at its first step."""

    def __init__(self, period=0.25, floor=0.0, seed=0):
        self.period, self.floor, self.seed = float(period), float(floor), int(seed)
        self.name = f"gain_envelope_{period}"

    def apply_batch(self, x, sr, seeds=None):
        if seeds is None:
            seeds = [self.seed + i for i in range(x.B)]
        return rt.gain_envelope(x, seeds, 0, 0, int(self.period * sr), self.floor)


@register
class BandFilter(Attack):
    """EXTENSION (not in the reference, parity unpinned): the embed loop's band_filter operator at fixed edges, applied after
    embedding: a zero-phase windowed-sinc FIR of 255 taps (embedding.loop_attacks.filter_taps), response "lowpass" or "highpass"
    at freq Hz, "bandpass" or "bandstop" between freq and freq_hi Hz.  The Butterworth classes above are what the loop's kind
    is measured against; this one is its own model."""

    def __init__(self, response, freq, freq_hi=None):
        from .embedding.loop_attacks import RESPONSES
        if response not in RESPONSES:
            raise ValueError(f"BandFilter: response = {response!r}; available: {list(RESPONSES)}")
        band = RESPONSES[response] >= 4
        if band != (freq_hi is not None):
            raise ValueError(f"BandFilter: {response} takes freq{' and freq_hi' if band else ' alone'}")
        self.response, self.freq, self.freq_hi = response, float(freq), float(freq if freq_hi is None else freq_hi)
        if not (np.isfinite(self.freq) and np.isfinite(self.freq_hi) and 0.0 < self.freq <= self.freq_hi):
            raise ValueError(f"BandFilter: 0 < freq <= freq_hi, both finite, are required; got {freq!r}, {freq_hi!r}")
        self.name = f"band_filter_{response}_{freq}" + (f"_{freq_hi}" if band else "")

    def apply_batch(self, x, sr):
        from .embedding.loop_attacks import MAX_EDGE, RESPONSES, filter_edge
        c1, c2 = filter_edge(self.freq, sr), filter_edge(self.freq_hi, sr)
        if not 1 <= c1 <= c2 <= MAX_EDGE:
            raise ValueError(f"BandFilter: {self.freq} .. {self.freq_hi} Hz does not lie inside (0, Nyquist) at {sr} Hz")
        return rt.band_filter(x, RESPONSES[self.response], c1, c2)


@register
class FrequencyShift(Attack):
    """EXTENSION (not in the reference, parity unpinned): the embed loop's frequency_shift operator at a fixed shift, applied
    after embedding: every component moved by hz (positive: upwards) through the 255-tap Hilbert transformer
    (embedding.loop_attacks.hilbert_taps), from the start phase `phase` in turns.  Single-sideband modulation: neither a pitch
    shift nor a speed change.  The clip keeps its length."""

    def __init__(self, hz, phase=0.0):
        self.hz, self.phase = float(hz), float(phase)
        if not (np.isfinite(self.hz) and np.isfinite(self.phase)):
            raise ValueError(f"FrequencyShift: hz and phase have to be finite; got {hz!r}, {phase!r}")
        self.name = f"frequency_shift_{hz}"

    def apply_batch(self, x, sr):
        from .embedding.loop_attacks import MAX_SHIFT, PHASE_ONE, shift_increment
        d = shift_increment(self.hz, sr)
        if abs(d) > MAX_SHIFT:
            raise ValueError(f"FrequencyShift: {self.hz} Hz lies beyond +-{sr / 16:g} Hz, the widest shift at {sr} Hz")
        return rt.frequency_shift(x, d, int(round((self.phase % 1.0) * PHASE_ONE)) % PHASE_ONE)


def _excerpt_bounds(name, seconds, start_seconds, x, sr):
    """(starts, lengths) in samples of the excerpt of every clip of x: int(start_seconds * sr) and int(seconds * sr), inside it."""
    s, L = int(start_seconds * sr), int(seconds * sr)
    if L < 1 or any(s + L > n for n in x.lengths):
        raise ValueError(f"{name}: the excerpt [{s}, {s + L}) at {sr} Hz does not lie inside clips of {list(x.lengths)} samples")
    return [s] * x.B, [L] * x.B


@register
class Excerpt(Attack):
    """EXTENSION (not in the reference, parity unpinned; its Cropout above drops the head only): the true excerpt, a shorter
    clip: the int(seconds * sr) samples from int(start_seconds * sr) on, and nothing else.  What the embed loop's excerpt kind
    is measured against; a detector needs more than 512 samples."""

    def __init__(self, seconds, start_seconds=0.0):
        self.seconds, self.start_seconds = float(seconds), float(start_seconds)
        if not (np.isfinite(self.seconds) and np.isfinite(self.start_seconds) and self.seconds > 0.0 and self.start_seconds >= 0.0):
            raise ValueError(f"Excerpt: seconds > 0 and start_seconds >= 0, both finite, are required; got {seconds!r}, {start_seconds!r}")
        self.name = f"excerpt_{seconds}_at_{start_seconds}"

    def apply_batch(self, x, sr):
        starts, lengths = _excerpt_bounds("Excerpt", self.seconds, self.start_seconds, x, sr)
        head = rt.segment_cut(x, [0] * x.B, starts, zero_fill=False)                        # x[start:]
        return rt.segment_cut(head, lengths, [n - L for n, L in zip(head.lengths, lengths)], zero_fill=False)


@register
class ExcerptTile(Attack):
    """EXTENSION (not in the reference, parity unpinned): the embed loop's excerpt operator at fixed values, applied after
    embedding: the int(seconds * sr) samples from int(start_seconds * sr) on, repeated periodically until they fill the clip,
    which keeps its length (embedding.loop_attacks.excerpt_tile).  Excerpt above is what the loop's kind is measured against;
    this one is its own model."""

    def __init__(self, seconds, start_seconds=0.0):
        self.seconds, self.start_seconds = float(seconds), float(start_seconds)
        if not (np.isfinite(self.seconds) and np.isfinite(self.start_seconds) and self.seconds > 0.0 and self.start_seconds >= 0.0):
            raise ValueError(f"ExcerptTile: seconds > 0 and start_seconds >= 0, both finite, are required; got {seconds!r}, {start_seconds!r}")
        self.name = f"excerpt_tile_{seconds}_at_{start_seconds}"

    def apply_batch(self, x, sr):
        return rt.excerpt_tile(x, *_excerpt_bounds("ExcerptTile", self.seconds, self.start_seconds, x, sr))


@register
class TimeWarp(Attack):
    """EXTENSION (not in the reference, parity unpinned): the clip played at a speed that wanders inside it, piecewise linear
    between random breakpoints, each rate uniform in 1 +- depth.  Clip i draws the warp of seed + i that
    embedding.loop_attacks.apply_chain specifies at step 0, entry 0: what a {"kind": "time_warp", "depth": depth, "period": period}
    entry of the embed loop applies at its first step.  The clip keeps its length."""

    def __init__(self, depth=0.04, period=(0.032, 0.512), seed=0):
        from .embedding.loop_attacks import parse_chain
        self.entry = parse_chain([{"kind": "time_warp", "depth": depth, "period": period}])[0]      # its refusals are this one's
        self.seed = int(seed)
        self.name = f"time_warp_{depth}"

    def apply_batch(self, x, sr, seeds=None):
        from .embedding import loop_attacks as la
        if seeds is None:
            seeds = [self.seed + i for i in range(x.B)]
        D = la.warp_range(self.entry, sr)[2]
        es, phs, rates = [], [], []
        for sd, n in zip(seeds, x.lengths):
            e, ph = la.warp_draw(self.entry, la.entry_draw(int(sd) & 0xFFFFFFFF, 0, 0), sr)
            es.append(e)
            phs.append(ph)
            rates.append(la.warp_rates(sd, 0, 0, la.warp_breakpoints(n, e), D))
        return rt.time_warp(x, es, phs, rates)


@register
class Flutter(Attack):
    """EXTENSION (not in the reference, parity unpinned): wow (a few tenths of a hertz to a few hertz) and flutter (above):
    the clip played at the speed 1 + depth sin(2 pi hz t + phase), through the embed loop's time_warp operator at the finest
    breakpoints it has, 256 samples apart: m_k = round(65536 depth sin(2 pi hz 256 k / sr + phase)).  The clip keeps its
    length."""

    def __init__(self, depth, hz, phase=0.0):
        self.depth, self.hz, self.phase = float(depth), float(hz), float(phase)
        if not (np.isfinite(self.depth) and np.isfinite(self.hz) and np.isfinite(self.phase) and 0.0 < self.depth < 0.1 and self.hz > 0.0):
            raise ValueError(f"Flutter: 0 < depth < 0.1 and hz > 0, all finite, are required; got {depth!r}, {hz!r}, {phase!r}")
        self.name = f"flutter_{depth}_{hz}"

    def rates(self, n, sr):
        """The rate offsets m_k of a clip of n samples at sr Hz."""
        from .embedding.loop_attacks import warp_breakpoints
        k = np.arange(warp_breakpoints(n, 8), dtype=np.float64)
        return np.round(65536.0 * self.depth * np.sin(2.0 * np.pi * self.hz * 256.0 * k / sr + self.phase)).astype(np.int64)

    def apply_batch(self, x, sr):
        return rt.time_warp(x, 8, 0, [self.rates(n, sr) for n in x.lengths])


def _scale(x: "rt.Ragged", gains) -> "rt.Ragged":
    """x times one gain curve per clip (torch tensors on x's device), float32."""
    data = x.data.float()
    return rt.Ragged(torch.cat([data[o:o + n] * g.to(data.dtype) for o, n, g in zip(x.offsets, x.lengths, gains)]), x.lengths)


@register
class Fade(Attack):
    """EXTENSION (not in the reference, parity unpinned): a linear fade-in over the first seconds_in and / or a linear fade-out
    over the last seconds_out of the clip.  A side that is not given is not faded; None means the whole clip for that side:
    Fade(seconds_in=None) rises over the whole clip, Fade(seconds_out=0.5) falls over the last half second.  At least one side
    is given.  Plain torch on the ragged buffer, on purpose: what the loop's gain_envelope entry buys is measured with an
    operator its model does not contain."""
    _ABSENT = object()

    def __init__(self, seconds_in=_ABSENT, seconds_out=_ABSENT):
        if seconds_in is Fade._ABSENT and seconds_out is Fade._ABSENT:
            raise ValueError("Fade: at least one of seconds_in and seconds_out is required (None: the whole clip)")
        for v in (seconds_in, seconds_out):
            if v is not None and v is not Fade._ABSENT and not (np.isfinite(v) and v > 0.0):
                raise ValueError(f"Fade: seconds have to be finite and > 0, or None; got {v!r}")
        self.seconds_in, self.seconds_out = seconds_in, seconds_out
        side = lambda v: "none" if v is Fade._ABSENT else ("all" if v is None else v)
        self.name = f"fade_in_{side(seconds_in)}_out_{side(seconds_out)}"

    def _samples(self, v, n, sr):
        return 0 if v is Fade._ABSENT else (n if v is None else max(1, min(n, int(v * sr))))

    def gain(self, n, sr, device):
        t = torch.arange(n, dtype=torch.float64, device=device)
        g = torch.ones(n, dtype=torch.float64, device=device)
        k_in, k_out = self._samples(self.seconds_in, n, sr), self._samples(self.seconds_out, n, sr)
        if k_in > 0:
            g = g * torch.clamp(t / k_in, max=1.0)
        if k_out > 0:
            g = g * torch.clamp((n - 1 - t) / k_out, max=1.0)
        return g.float()

    def apply_batch(self, x, sr):
        return _scale(x, [self.gain(n, sr, x.data.device) for n in x.lengths])


@register
class Tremolo(Attack):
    """EXTENSION (not in the reference, parity unpinned): amplitude modulation 1 - depth / 2 * (1 + sin(2 pi rate_hz t)), t in
    seconds from the clip's start: the gain swings between 1 and 1 - depth.  Plain torch, as Fade and for its reason."""

    def __init__(self, rate_hz, depth):
        self.rate_hz, self.depth = float(rate_hz), float(depth)
        if not (np.isfinite(self.rate_hz) and self.rate_hz > 0.0 and 0.0 <= self.depth <= 1.0):
            raise ValueError(f"Tremolo: rate_hz > 0 and 0 <= depth <= 1 are required; got {rate_hz!r}, {depth!r}")
        self.name = f"tremolo_{rate_hz}Hz_{depth}"

    def gain(self, n, sr, device):
        t = torch.arange(n, dtype=torch.float64, device=device) / sr
        return (1.0 - self.depth / 2.0 * (1.0 + torch.sin(2.0 * np.pi * self.rate_hz * t))).float()

    def apply_batch(self, x, sr):
        return _scale(x, [self.gain(n, sr, x.data.device) for n in x.lengths])


@register
class SpeedChange(Attack):
    """EXTENSION (not in the reference, parity unpinned): the clip played fast or slow by `cents` (pitch and duration change
    together, as under a sample-rate mismatch): Catmull-Rom resampling at the fixed ratio R / 65536,
    R = 65536 + round(65536 (2^(cents / 1200) - 1)), as embedding.loop_attacks.speed_change specifies it.  A true speed
    change: a clip of n samples comes out ((n - 1) << 16) // R + 1 long.  Inside the embed loop the same operator keeps the
    clip's length ({"kind": "speed_change", "cents": ...})."""

    def __init__(self, cents=50.0):
        self.cents = float(cents)
        self.m = int(round(65536.0 * (2.0 ** (self.cents / 1200.0) - 1.0)))
        self.name = f"speed_{cents}"

    def apply_batch(self, x, sr):
        from .embedding.loop_attacks import speed_length
        return rt.speed_change(x, [self.m] * x.B, out_lengths=[speed_length(n, self.m) for n in x.lengths])


@register
class OverlapAddStretch(Attack):
    """EXTENSION (not in the reference, parity unpinned): the clip stretched in time at `rate` (above 1: faster and shorter, the
    pitch kept) by plain overlap-add of Hann-windowed segments at the fixed rate Q / 65536, Q = 65536 + round(65536 (rate - 1)),
    as embedding.loop_attacks.time_stretch specifies it.  A true stretch: a clip of n samples comes out
    ((n - 1) << 16) // Q + 1 long.  Inside the embed loop the same operator keeps the clip's length
    ({"kind": "time_stretch", "rate": ...}).  TimeStretch is the phase vocoder, built differently."""

    def __init__(self, rate=1.05):
        self.rate = float(rate)
        self.m = int(round(65536.0 * (self.rate - 1.0)))
        self.name = f"ola_{rate}"

    def apply_batch(self, x, sr):
        from .embedding.loop_attacks import stretch_length
        return rt.stretch_ola(x, [self.m] * x.B, out_lengths=[stretch_length(n, self.m) for n in x.lengths])


@register
class OverlapAddPitchShift(Attack):
    """EXTENSION (not in the reference, parity unpinned): the clip's pitch moved by `cents` at its own duration, as the
    resampling at R / 65536, R = 65536 + round(65536 (2^(cents / 1200) - 1)), of the plain overlap-add stretch at the coupled
    rate round(2^32 / R) / 65536, in one launch, as embedding.loop_attacks.pitch_shift specifies it.  The output is as long as
    the input.  Inside the embed loop it is the chain entry {"kind": "pitch_shift", "cents": ...}.  PitchShift is the phase
    vocoder, built differently."""

    def __init__(self, cents=50.0):
        self.cents = float(cents)
        self.m = int(round(65536.0 * (2.0 ** (self.cents / 1200.0) - 1.0)))
        self.name = f"ola_ps_{cents}"

    def apply_batch(self, x, sr):
        return rt.pitch_shift_ola(x, [self.m] * x.B)


@register
class MP3Surrogate(Attack):
    """EXTENSION (not in the reference; BASELINE.json north_star): MP3-like quantisation surrogate
    -- STFT -> per-frame log-magnitude quantisation (`step_db` grid, bins more than `-floor_db` below
    the frame maximum dropped) -> iSTFT.  It is NOT a codec and does not replace the reference's
    ffmpeg-based MP3Compression (out of scope: external binary).  Specified by
    oracle/aware_oracle.py::mp3_surrogate_attack -- parity unpinned.  Output length 256*(T-1)."""

    def __init__(self, step_db=1.5, floor_db=-60.0):
        self.step_db, self.floor_db = float(step_db), float(floor_db)
        self.name = f"mp3_surrogate_{step_db}dB"

    def apply_batch(self, x, sr):
        from .utils.audio import default_plan
        plan = default_plan()
        batch = x.batch()
        spec = rt.stft(plan, batch, x.data, normalize=False)
        rt.spectral_quantize(spec, self.step_db, self.floor_db)
        y = rt.istft(plan, batch, spec, normalize=False)
        return rt.Ragged(y, batch.out_lengths)


@register
class TimeStretch(Attack):
    """EXTENSION in place of scripts/attacks.py:208-228 (pyrubberband -> rubberband binary, absent): phase-vocoder
    time-scale modification on the STFT kernels.  rate > 1: faster / shorter, rate < 1: slower / longer.  Specified by
    oracle/aware_oracle.py::time_stretch_attack -- parity with rubberband unpinned.  Output length 256*(ceil(T/rate)-1)."""

    def __init__(self, rate=1.0):
        self.rate = float(rate)
        self.name = f"ts_{rate}"

    def apply_batch(self, x, sr):
        from .utils.audio import default_plan
        return rt.time_stretch(default_plan(), x, self.rate)


@register
class PitchShift(Attack):
    """EXTENSION in place of scripts/attacks.py:231-252: pitch shift by `cents`/100 semitones (the reference's own
    unit conversion, :249) = phase-vocoder stretch by 2^(semitones/12) followed by polyphase resampling back to the
    original duration.  Specified by oracle/aware_oracle.py::pitch_shift_attack -- parity with rubberband unpinned."""

    def __init__(self, cents=5):
        self.cents = cents
        self.name = f"ps_{cents}"

    def ratio(self):
        from fractions import Fraction
        factor = 2.0 ** ((self.cents / 100.0) / 12.0)
        fr = Fraction(1.0 / factor).limit_denominator(512)          # resampling ratio up/down ~ 1/factor
        return factor, fr.numerator, fr.denominator

    def apply_batch(self, x, sr):
        from .utils.audio import default_plan
        factor, up, down = self.ratio()
        y = rt.time_stretch(default_plan(), x, 1.0 / factor)
        return y if up == down else resample_poly_batch(y, up, down)


def reference_attack_list():
    """The subset of the harness's 22-entry list (scripts/test.py:15-18) that runs here."""
    return [PCMBitDepthConversion(8), PCMBitDepthConversion(12), PCMBitDepthConversion(16), PCMBitDepthConversion(24),
            DeleteSamples(0.1), DeleteSamples(0.15), DeleteSamples(0.2), Resample(), RandomBandstop(),
            SampleSupression(0.1), SampleSupression(0.25), LowPassFilter(), HighPassFilter()]


def config3_attack_stack():
    """BASELINE.json config 3: resample 44.1k<->16k + lowpass + Gaussian noise + quantisation."""
    return [Resample(), LowPassFilter(), GaussianNoise(20.0), PCMBitDepthConversion(16)]
