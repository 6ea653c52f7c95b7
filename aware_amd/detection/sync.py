"""Offset search in detection (EXTENSION, parity unpinned: the reference detects at the clip's own start only).

The detector network pools pairs of frames of hop 256 first (initial pool (2, 2)), so its read-out has a period of
SYNC_PERIOD = 512 samples in where the clip starts: a clip whose first d samples are gone re-pairs the pooled frames and reads
worse the nearer d mod 512 is to 256.  With sync_search = n the detector reads n views of every clip, view j with a further
e_j = j * (512 / n) samples dropped, and keeps the view it is most confident about.  `sync_select` is the specification the
device kernel (csrc/sync_kernels.hip, aware_sync_select) is tested against:

    c_j = mean_l |v[b][j][l] - centre| in float32,  j* = the smallest j with the largest c_j,  out[b] = v[b][j*]

centre is 0.5 for a sigmoid read-out and 0 otherwise.

Speed search (EXTENSION as well).  A clip that was played at another speed (resampled: pitch and tempo
move together) loses its bits, and reads them again once it is played back at the inverse speed.  With speed_search on, the
detector reads every clip at 2 K + 1 candidate speeds and keeps the most confident view, by the same rule:

    delta = floor(65536 step_percent / 100 + 0.5),  K = floor(max_percent / step_percent + 1e-9),
    m_0 = 0,  m_{2i-1} = -i delta,  m_{2i} = +i delta,  i = 1 .. K          (ordered by |m|: a tie prefers the plain read)
    view j of a clip of n samples = loop_attacks.speed_change(x, m_j, speed_length(n, m_j))

the existing operator (Catmull-Rom at the 16.16 positions i (65536 + m_j)) at the length that keeps every position inside the
clip.  The device writes all views in one launch (csrc/speed_search_kernels.hip, aware_speed_views).  With the offset search on
as well, every speed view is read at the n sync offsets, and `speed_select` states the selection over all of them.

Shift search (EXTENSION as well).  A clip whose every component was moved by the same number of Hz
(single-sideband modulation: a detuned receiver, an analogue carrier) loses its bits, a quarter to a third of them at 20 Hz and
all of them at 50 Hz, and reads them again once it is moved back.  With shift_search on, the detector reads every clip at
2 K + 1 candidate shifts and keeps the most confident view, by the same rule:

    delta = loop_attacks.shift_increment(step_hz, sample_rate),  K = floor(max_hz / step_hz + 1e-9),  K delta <= MAX_SHIFT,
    d_0 = 0,  d_{2i-1} = -i delta,  d_{2i} = +i delta,  i = 1 .. K          (ordered by |d|: a tie prefers the plain read)
    view j of a clip = loop_attacks.frequency_shift(x, d_j, 0)

the existing operator (the 255-tap Hilbert transformer and the integer phase (i d_j) mod 2^20) from the start phase 0; every
view has the clip's length.  The device writes all views in one launch (csrc/shift_search_kernels.hip, aware_shift_views), the
Hilbert transform once per clip.  `shift_select` is `speed_select`'s rule, sync views included.  The search is not served
together with the speed search: the product of the two grids is not read."""
from __future__ import annotations

import math

import numpy as np

SYNC_PERIOD = 512                       # hop 256 times the (2, 2) initial pool
SYNC_CHOICES = (2, 4, 8, 16, 32, 64)
SYNC_MAX_ROWS = 4096                    # views per aware_detect call: larger searches are chunked on the host
SPEED_MAX_VIEWS = 63                    # speed views per clip: the second round of aware_sync_select takes n <= 64
SPEED_MAX_SAMPLES = 1 << 30             # samples of the views of one aware_speed_views call
SPEED_STEP_DEFAULT = 0.5                # percent: the confidence peak is about +-0.35 % wide at half height
SHIFT_MAX_VIEWS = 63                    # shift views per clip: the second round of aware_sync_select takes n <= 64
SHIFT_MAX_SAMPLES = 1 << 30             # samples of the views of one aware_shift_views call
SHIFT_STEP_DEFAULT = 10.0               # Hz: a residual of 5 Hz keeps 0.161 of the confidence 0.264 at 0 Hz, one of 13 Hz 0.044


def check_sync_search(n) -> int:
    """The number of views: 0 for off (None, 0 or 1), one of SYNC_CHOICES otherwise; ValueError for anything else."""
    if n is None:
        return 0
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
        raise ValueError(f"sync_search = {n!r}: 0 (off) or one of {SYNC_CHOICES} is expected")
    n = int(n)
    if n in (0, 1):
        return 0
    if n not in SYNC_CHOICES:
        raise ValueError(f"sync_search = {n}: 0 (off) or one of {SYNC_CHOICES} is expected")
    return n


def sync_offsets(n: int) -> list[int]:
    """e_j = j * (512 / n), j = 0 .. n - 1: the samples view j drops at the clip's start."""
    n = check_sync_search(n) or 1
    return [j * (SYNC_PERIOD // n) for j in range(n)]


def sync_views(lengths, n: int):
    """(view lengths, view offsets inside their clip), clip-major, of the n views of clips `lengths` long.  ValueError for a
    clip whose shortest view would have 512 samples or fewer (the STFT's reflect padding needs more)."""
    offs = sync_offsets(n)
    for b, nb in enumerate(lengths):
        if int(nb) - offs[-1] <= SYNC_PERIOD:
            raise ValueError(f"sync_search = {n}: clip {b} has {int(nb)} samples; its shortest view ({int(nb) - offs[-1]}) needs "
                             f"more than {SYNC_PERIOD}")
    return [int(nb) - e for nb in lengths for e in offs], [e for _ in lengths for e in offs]


def sync_select(values, n: int, centre: float = 0.0):
    """values [B * n, L] (numpy or torch, clip-major: the n views of clip 0, then those of clip 1, ...) ->
    (out [B, L] float32: per clip the view with the largest c_j = mean_l |v_jl - centre|, the smallest j on a tie;
    index [B] int32; confidence [B] float32).  numpy in, numpy out; torch in, torch out."""
    is_torch = not isinstance(values, np.ndarray) and hasattr(values, "detach")
    v = values.detach().cpu().numpy() if is_torch else np.asarray(values)
    v = np.ascontiguousarray(v, dtype=np.float32)
    n = int(n)
    if v.ndim != 2 or n < 1 or v.shape[0] == 0 or v.shape[0] % n:
        raise ValueError(f"sync_select: values [B * n, L] with n = {n} are required; got {v.shape}")
    B, L = v.shape[0] // n, v.shape[1]
    v = v.reshape(B, n, L)
    conf = np.abs(v - np.float32(centre)).mean(axis=-1, dtype=np.float32)           # [B, n]
    idx = np.argmax(conf, axis=1).astype(np.int32)                                  # the first of equal maxima
    out = v[np.arange(B), idx]
    best = conf[np.arange(B), idx]
    if is_torch:
        import torch
        dev = values.device
        return torch.as_tensor(out, device=dev), torch.as_tensor(idx, device=dev), torch.as_tensor(best, device=dev)
    return out, idx, best


# ---- speed search -------------------------------------------------------------------------------------------------------------------
def check_speed_search(search):
    """None for off (None, 0, False or {}), {"max_percent", "step_percent"} in floats otherwise.  A number is max_percent with
    step_percent = 0.5.  ValueError for anything else: values that are not finite numbers, 0.05 <= step_percent <= 2 and
    step_percent <= max_percent <= 20 violated, an unknown key, more than 63 views."""
    def number(v, what):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
            raise ValueError(f"speed_search: {what} = {v!r}: a finite number is expected")
        return float(v)

    if search is None or search is False:
        return None
    if isinstance(search, dict):
        if not search:
            return None
        unknown = sorted(set(search) - {"max_percent", "step_percent"})
        if unknown or "max_percent" not in search:
            raise ValueError(f"speed_search = {search!r}: the keys are max_percent and, optionally, step_percent")
        mx = number(search["max_percent"], "max_percent")
        step = number(search.get("step_percent", SPEED_STEP_DEFAULT), "step_percent")
    else:
        mx, step = number(search, "max_percent"), SPEED_STEP_DEFAULT
        if mx == 0.0:
            return None
    if not 0.05 <= step <= 2.0:
        raise ValueError(f"speed_search: step_percent = {step}: 0.05 <= step_percent <= 2 is expected")
    if not step <= mx <= 20.0:
        raise ValueError(f"speed_search: max_percent = {mx}: step_percent = {step} <= max_percent <= 20 is expected")
    views = 2 * int(math.floor(mx / step + 1e-9)) + 1
    if views > SPEED_MAX_VIEWS:
        raise ValueError(f"speed_search: max_percent = {mx} at step_percent = {step} is {views} views; at most {SPEED_MAX_VIEWS}")
    return {"max_percent": mx, "step_percent": step}


def speed_offsets(search) -> list[int]:
    """The speed offsets m_j of the views, ordered by |m|: [0, -delta, +delta, -2 delta, ...]; [0] where the search is off."""
    s = check_speed_search(search)
    if s is None:
        return [0]
    delta = int(math.floor(65536.0 * s["step_percent"] / 100.0 + 0.5))
    k = int(math.floor(s["max_percent"] / s["step_percent"] + 1e-9))
    return [0] + [sign * i * delta for i in range(1, k + 1) for sign in (-1, 1)]


def speed_of(m: int) -> float:
    """The speed a received clip was played at, if the view at the offset m restores it: 65536 / (65536 + m)."""
    return 65536.0 / (65536.0 + int(m))


def speed_views(lengths, search, sync_n: int = 0) -> list[int]:
    """The view lengths speed_length(n_b, m_j), clip-major, of clips `lengths` long.  ValueError, naming the clip, where a
    clip's shortest view, less the largest offset of the offset search sync_n, would have 512 samples or fewer (the STFT's
    reflect padding needs more), or where the views of one clip, each padded to a multiple of four samples, exceed 2^30."""
    from ..embedding.loop_attacks import speed_length
    ms = speed_offsets(search)
    drop = sync_offsets(sync_n)[-1]
    out = []
    for b, nb in enumerate(lengths):
        v = [speed_length(int(nb), m) for m in ms] if int(nb) >= 1 else [0] * len(ms)
        if min(v) - drop <= SYNC_PERIOD:
            raise ValueError(f"speed_search: clip {b} has {int(nb)} samples; its shortest view ({min(v)}"
                             + (f", less {drop} for sync_search = {sync_n}" if drop else "") + f") needs more than {SYNC_PERIOD}")
        if sum((n + 3) // 4 * 4 for n in v) > SPEED_MAX_SAMPLES:
            raise ValueError(f"speed_search: the {len(ms)} views of clip {b} ({int(nb)} samples) exceed 2^30 samples")
        out += v
    return out


def speed_select(values, n_speed: int, n_sync: int = 0, centre: float = 0.0):
    """values [B * n_speed * max(n_sync, 1), L], clip-major, then the speed view, then the sync view -> (out [B, L] float32:
    per clip the row with the largest mean_l |v - centre| in float32, the smallest flat index on a tie; that flat index
    idx_speed * n_sync + idx_sync [B] int32; that mean [B] float32).  It equals two rounds of sync_select, over the sync views
    of every (clip, speed view) and then over the speed views, which is how the device selects."""
    return sync_select(values, int(n_speed) * max(int(n_sync), 1), centre)


# ---- shift search -------------------------------------------------------------------------------------------------------------------
def check_shift_search(search):
    """None for off (None, 0, False or {}), {"max_hz", "step_hz"} in floats otherwise.  A number is max_hz with step_hz = 10.
    ValueError for anything else: values that are not finite numbers, 1 <= step_hz <= 20 and step_hz <= max_hz violated, an
    unknown key, more than 63 views.  (max_hz <= sample_rate / 16 is shift_offsets' to check: it needs the sample rate.)"""
    def number(v, what):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
            raise ValueError(f"shift_search: {what} = {v!r}: a finite number is expected")
        return float(v)

    if search is None or search is False:
        return None
    if isinstance(search, dict):
        if not search:
            return None
        unknown = sorted(set(search) - {"max_hz", "step_hz"}, key=str)
        if unknown or "max_hz" not in search:
            raise ValueError(f"shift_search = {search!r}: the keys are max_hz and, optionally, step_hz")
        mx = number(search["max_hz"], "max_hz")
        step = number(search.get("step_hz", SHIFT_STEP_DEFAULT), "step_hz")
    else:
        mx, step = number(search, "max_hz"), SHIFT_STEP_DEFAULT
        if mx == 0.0:
            return None
    if not 1.0 <= step <= 20.0:
        raise ValueError(f"shift_search: step_hz = {step}: 1 <= step_hz <= 20 is expected")
    if not step <= mx:
        raise ValueError(f"shift_search: max_hz = {mx}: step_hz = {step} <= max_hz is expected")
    views = 2 * int(math.floor(mx / step + 1e-9)) + 1
    if views > SHIFT_MAX_VIEWS:
        raise ValueError(f"shift_search: max_hz = {mx} at step_hz = {step} is {views} views; at most {SHIFT_MAX_VIEWS}")
    return {"max_hz": mx, "step_hz": step}


def shift_offsets(search, sample_rate: int) -> list[int]:
    """The shifts d_j of the views in units of sample_rate / 2^20 Hz, ordered by |d|: [0, -delta, +delta, -2 delta, ...] with
    delta = shift_increment(step_hz, sample_rate); [0] where the search is off.  ValueError where K delta exceeds MAX_SHIFT
    (max_hz above sample_rate / 16) or delta is 0."""
    from ..embedding.loop_attacks import MAX_SHIFT, shift_increment
    s = check_shift_search(search)
    if s is None:
        return [0]
    delta = shift_increment(s["step_hz"], int(sample_rate))
    k = int(math.floor(s["max_hz"] / s["step_hz"] + 1e-9))
    if delta < 1 or k * delta > MAX_SHIFT:
        raise ValueError(f"shift_search: max_hz = {s['max_hz']} at step_hz = {s['step_hz']} is +-{k * delta} in units of "
                         f"{int(sample_rate)} / 2^20 Hz, outside 1..{MAX_SHIFT} (+-{int(sample_rate) / 16:g} Hz)")
    return [0] + [sign * i * delta for i in range(1, k + 1) for sign in (-1, 1)]


def shift_of(d: int, sample_rate: int) -> float:
    """The shift in Hz a received clip carried, if the view at d restores it: -d sample_rate / 2^20."""
    return -int(d) * float(sample_rate) / float(1 << 20)


def shift_views(lengths, search, sample_rate: int, sync_n: int = 0) -> list[int]:
    """The view lengths, clip-major, of clips `lengths` long: every view of clip b has n_b samples.  ValueError, naming the
    clip, where n_b less the largest offset of the offset search sync_n is 512 or fewer (the STFT's reflect padding needs
    more), or where the views of one clip, each padded to a multiple of four samples, exceed 2^30."""
    nv = len(shift_offsets(search, sample_rate))
    drop = sync_offsets(sync_n)[-1]
    out = []
    for b, nb in enumerate(lengths):
        nb = int(nb)
        if nb - drop <= SYNC_PERIOD:
            raise ValueError(f"shift_search: clip {b} has {nb} samples; its views ({nb}"
                             + (f", less {drop} for sync_search = {sync_n}" if drop else "") + f") need more than {SYNC_PERIOD}")
        if nv * ((nb + 3) // 4 * 4) > SHIFT_MAX_SAMPLES:
            raise ValueError(f"shift_search: the {nv} views of clip {b} ({nb} samples) exceed 2^30 samples")
        out += [nb] * nv
    return out


def shift_select(values, n_shift: int, n_sync: int = 0, centre: float = 0.0):
    """speed_select's rule for the shift search: values [B * n_shift * max(n_sync, 1), L], clip-major, then the shift view, then
    the sync view -> (out [B, L], the flat index idx_shift * n_sync + idx_sync [B] int32, the confidence [B] float32)."""
    return speed_select(values, n_shift, n_sync, centre)


# ---- scanning long recordings -------------------------------------------------------------------------------------------------------
# (EXTENSION)  A long file in which only a part is marked reads nothing as a whole.  The scan reads it in
# windows, every window at the n sync offsets, keeps the most confident view per window (scan_select) and joins marked windows
# that agree on their bits into runs (scan_segments): one payload per run.  These functions are the specification the device
# kernels (csrc/scan_kernels.hip, aware_scan_select and aware_scan_segments) are tested against.
SCAN_WINDOW_SECONDS = 1.0
SCAN_HOP = 4096
SCAN_SYNC = 8
SCAN_MAX_SEGMENTS = 16
SCAN_MIN_CONFIDENCE = 0.06              # 2.2 x the largest of 76 unmarked windows (0.0270); where a half-overlapping window reads
SCAN_MAX_BITS = 512                     # L of aware_scan_select / aware_scan_segments
SCAN_KEYS = ("window_seconds", "hop_samples", "min_confidence", "max_segments")


def check_scan(window_seconds=SCAN_WINDOW_SECONDS, hop_samples=SCAN_HOP, min_confidence=SCAN_MIN_CONFIDENCE,
               max_segments=SCAN_MAX_SEGMENTS, max_flip=None, sample_rate: int = 16000) -> dict:
    """The scan's parameters, checked: {"window_seconds", "hop_samples", "min_confidence", "max_segments", "max_flip",
    "window"} with `window` in samples at sample_rate.  ValueError, naming the key, for: a window_seconds that is not a
    finite number or gives a window of 512 samples or fewer (or of 2^30 or more), a hop_samples that is not a positive
    multiple of 512, a min_confidence that is not a finite number, a max_segments that is not an integer >= 1, a max_flip
    that is neither None (n_bits // 4 is then used) nor an integer >= 0."""
    def number(v, key):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
            raise ValueError(f"scan: {key} = {v!r}: a finite number is expected")
        return float(v)

    def integer(v, key, lo):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < lo:
            raise ValueError(f"scan: {key} = {v!r}: an integer >= {lo} is expected")
        return int(v)

    ws = number(window_seconds, "window_seconds")
    window = int(round(ws * int(sample_rate))) if 0.0 < ws * int(sample_rate) < float(1 << 30) else 0
    if window <= SYNC_PERIOD:
        raise ValueError(f"scan: window_seconds = {window_seconds!r}: a window of more than {SYNC_PERIOD} and fewer than 2^30 "
                         f"samples at {int(sample_rate)} Hz is expected")
    hop = integer(hop_samples, "hop_samples", 1)
    if hop % SYNC_PERIOD:
        raise ValueError(f"scan: hop_samples = {hop}: a positive multiple of {SYNC_PERIOD} is expected")
    return {"window_seconds": ws, "hop_samples": hop, "min_confidence": number(min_confidence, "min_confidence"),
            "max_segments": integer(max_segments, "max_segments", 1),
            "max_flip": None if max_flip is None else integer(max_flip, "max_flip", 0), "window": window}


def check_scan_card(scan) -> dict:
    """The card key `scan`: None or {} for the defaults, or a dict with some of SCAN_KEYS -> all four, checked by check_scan.
    ValueError for anything else, naming the key."""
    if scan is None:
        scan = {}
    if not isinstance(scan, dict):
        raise ValueError(f"scan = {scan!r}: a mapping with some of the keys {SCAN_KEYS} is expected")
    unknown = sorted(set(scan) - set(SCAN_KEYS), key=str)
    if unknown:
        raise ValueError(f"scan: unknown key {unknown[0]!r}: the keys are {SCAN_KEYS}")
    checked = check_scan(**scan)
    return {k: checked[k] for k in SCAN_KEYS}


def scan_windows(n_samples: int, window: int, hop: int, n_sync: int, index: int = 0):
    """(starts, length): the windows of a file of n_samples.  With e_max the largest of sync_offsets(n_sync), windows of
    `window` samples start at 0, hop, 2 hop, ... while start + e_max + window <= n_samples, and one more at
    n_samples - window - e_max where that start is not on the grid: view j of a window reads `length` samples from
    start + e_j.  A file shorter than window + e_max is one window of n_samples - e_max samples.  ValueError for a hop that is
    no positive multiple of 512, a window of 512 samples or fewer, and, naming the file by `index`, a file with
    n_samples - e_max <= 512 (the STFT's reflect padding needs more)."""
    n_samples, window, hop = int(n_samples), int(window), int(hop)
    e_max = sync_offsets(n_sync)[-1]
    if hop < 1 or hop % SYNC_PERIOD:
        raise ValueError(f"scan: hop_samples = {hop}: a positive multiple of {SYNC_PERIOD} is expected")
    if window <= SYNC_PERIOD:
        raise ValueError(f"scan: a window of {window} samples: more than {SYNC_PERIOD} are expected")
    if n_samples - e_max <= SYNC_PERIOD:
        raise ValueError(f"scan with sync_search = {n_sync}: file {index} has {n_samples} samples; its shortest view "
                         f"({n_samples - e_max}) needs more than {SYNC_PERIOD}")
    if n_samples < window + e_max:
        return [0], n_samples - e_max
    tail = n_samples - window - e_max
    starts = list(range(0, tail + 1, hop))
    if tail % hop:
        starts.append(tail)
    return starts, window


def pack_bits(bits) -> np.ndarray:
    """bits [W, L] bool -> [W, ceil(L / 32)] uint32, bit l of a row at bit l % 32 of word l // 32: aware_scan_select's words."""
    bits = np.asarray(bits, dtype=bool)
    W, L = bits.shape
    padded = np.zeros((W, (L + 31) // 32 * 32), dtype=np.uint64)
    padded[:, :L] = bits
    return (padded.reshape(W, -1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def scan_select(values, win_off, n_sync: int, centre: float = 0.0):
    """values [W * n_sync, L] (numpy), window-major, the n_sync views of each of the W = win_off[-1] windows of all files ->
    (win_values [W, L] float32, win_view [W] int32, win_conf [W] float32, bits [W, L] bool).  Per window,
    c_j = mean_l |v_jl - centre| as in sync_select, j* the smallest j with the largest c_j, win_conf = c_j*,
    win_values = v_j*, bits = win_values > centre.  A c_j that is NaN never wins; a window whose c_j are all NaN keeps view 0
    with win_conf = -1, as aware_sync_select does."""
    v = np.ascontiguousarray(np.asarray(values), dtype=np.float32)
    n, W = int(n_sync), int(np.asarray(win_off)[-1])
    if v.ndim != 2 or n < 1 or W < 1 or v.shape[0] != W * n:
        raise ValueError(f"scan_select: values [W * n_sync, L] with W = {W} and n_sync = {n} are required; got {v.shape}")
    L = v.shape[1]
    v = v.reshape(W, n, L)
    conf = np.abs(v - np.float32(centre)).mean(axis=-1, dtype=np.float32)           # [W, n]
    conf = np.where(np.isnan(conf), np.float32(-1.0), conf).astype(np.float32)
    view = np.argmax(conf, axis=1).astype(np.int32)                                 # the first of equal maxima
    out = v[np.arange(W), view]
    return out, view, conf[np.arange(W), view], out > np.float32(centre)


def scan_segments(C, V, win_off, centre: float, min_confidence: float, max_flip: int, max_segments: int, view=None,
                  dtype=np.float32):
    """Per file b, over its windows win_off[b] .. win_off[b + 1] of C [W] (win_conf) and V [W, L] (win_values): window w is
    marked where C_w >= min_confidence (a NaN is never marked); it continues the run of w - 1 where both are marked and
    bits_w = V_w > centre and bits_{w-1} differ in at most max_flip places, and a marked window opens a new run otherwise.
    -> a list over the files of (the true run count, the first max_segments runs), every run a dict of `first`, `last` and
    `peak` (window indices inside the file; the peak is the smallest w with the largest C_w), `view` (view[peak] where `view`
    is given, else 0), `confidence` (C_peak) and `values` [L]:

        values[l] = centre + (sum_w C_w (V_w[l] - centre)) / (sum_w C_w),  both sums in `dtype` over ascending w from zero.

    dtype = np.float64 is the yardstick the float32 sums are held against."""
    C = np.asarray(C, dtype=np.float32)
    V = np.asarray(V, dtype=np.float32)
    off = [int(o) for o in win_off]
    bits = V > np.float32(centre)
    ctr = dtype(centre)
    out = []
    for b in range(len(off) - 1):
        runs, count, prev = [], 0, False
        for w in range(off[b], off[b + 1]):
            marked = bool(C[w] >= np.float32(min_confidence))
            if marked and not (prev and int(np.count_nonzero(bits[w] != bits[w - 1])) <= int(max_flip)):
                count += 1
                if count <= int(max_segments):
                    runs.append([w, w])
            elif marked and count <= int(max_segments):
                runs[-1][1] = w
            prev = marked
        segs = []
        for first, last in runs:
            num, den = np.zeros(V.shape[1], dtype=dtype), dtype(0)
            for w in range(first, last + 1):
                num = num + dtype(C[w]) * (V[w].astype(dtype) - ctr)
                den = den + dtype(C[w])
            peak = first + int(np.argmax(C[first:last + 1]))
            segs.append({"first": first - off[b], "last": last - off[b], "peak": peak - off[b],
                         "view": int(view[peak]) if view is not None else 0, "confidence": float(C[peak]),
                         "values": (ctr + num / den).astype(dtype)})
        out.append((count, segs))
    return out
