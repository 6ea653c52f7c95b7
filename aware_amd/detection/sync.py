"""Offset search in detection (EXTENSION, parity unpinned: the reference detects at the clip's own start only).

The detector network pools pairs of frames of hop 256 first (initial pool (2, 2)), so its read-out has a period of
SYNC_PERIOD = 512 samples in where the clip starts: a clip whose first d samples are gone re-pairs the pooled frames and reads
worse the nearer d mod 512 is to 256.  With sync_search = n the detector reads n views of every clip, view j with a further
e_j = j * (512 / n) samples dropped, and keeps the view it is most confident about.  `sync_select` is the specification the
device kernel (csrc/sync_kernels.hip, aware_sync_select) is tested against:

    c_j = mean_l |v[b][j][l] - centre| in float32,  j* = the smallest j with the largest c_j,  out[b] = v[b][j*]

centre is 0.5 for a sigmoid read-out and 0 otherwise."""
from __future__ import annotations

import numpy as np

SYNC_PERIOD = 512                       # hop 256 times the (2, 2) initial pool
SYNC_CHOICES = (2, 4, 8, 16, 32, 64)
SYNC_MAX_ROWS = 4096                    # views per aware_detect call: larger searches are chunked on the host


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
