"""CPU tests of the device STOI's host side: exported symbols, workspace size, the frame arithmetic the kernels use against
the host function's own framing (aware_amd.metrics.audio._frames / _remove_silent_frames), the band edges and the
resampling filter.  No GPU compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from aware_amd.metrics import audio as M

STOI_SYMBOLS = ["aware_stoi_create", "aware_stoi_destroy", "aware_stoi_band_edges", "aware_stoi_frames",
                "aware_stoi_workspace_bytes", "aware_stoi"]


@pytest.fixture(scope="module")
def lib():
    from aware_amd._lib import build_library, load_library
    build_library()
    return load_library()


def test_symbols_exported_and_declared(lib):
    from aware_amd._lib import SIGNATURES, SOURCES
    header = open(os.path.join(ROOT, "include", "aware_hip.h")).read()
    declared = set(re.findall(r"\b(aware_[a-z0-9_]+)\s*\(", header))
    for name in STOI_SYMBOLS:
        assert name in declared and name in SIGNATURES and hasattr(lib, name), name
    assert "stoi_kernels.hip" in SOURCES
    assert lib.aware_version() >= 350
    from aware_amd import runtime as rt
    from aware_amd.metrics.audio import stoi_batch
    from aware_amd.pipeline import PipelineResult
    assert callable(rt.stoi) and callable(stoi_batch)
    assert "stoi" in PipelineResult.__dataclass_fields__ and PipelineResult.__dataclass_fields__["stoi"].default is None


def _frames_host(n):
    return len(M._frames(np.zeros(n), 256, 128, np.ones(256)))


BOUNDARY_LENGTHS = [0, 1, 128, 255, 256, 257, 258, 383, 384, 385, 386, 511, 512, 513, 640, 641, 4095, 4096, 4097, 30000,
                    30080, 30081, 100000, 600001]


@pytest.mark.parametrize("n", BOUNDARY_LENGTHS)
def test_first_stage_frame_count(lib, n):
    """range(0, n - 256, 128): no frame for n <= 256, and a frame that would end exactly at n is not taken."""
    from aware_amd import runtime as rt
    want = _frames_host(n)
    assert rt.stoi_frames(n) == want
    assert lib.aware_stoi_frames(n) == want
    if want:
        assert 128 * (want - 1) + 256 < n                    # the last frame ends inside the clip (the kernels' bound)
        assert 128 * want + 256 >= n                         # ... and one more would not


def test_frame_count_refuses_negative_length(lib):
    assert lib.aware_stoi_frames(-1) == -1


def _reframe_mirror(x, kept, w):
    """What stoi_bands_kernel builds: frame m of the overlap-added kept frames from kept frames m - 1, m, m + 1 only."""
    xf = [w * x[128 * f:128 * f + 256] for f in kept]
    rows = []
    for m in range(max(len(kept) - 1, 0)):
        fr = xf[m].copy()
        if m >= 1:
            fr[:128] += xf[m - 1][128:]
        fr[128:] += xf[m + 1][:128]
        rows.append(w * fr)
    return np.array(rows) if rows else np.zeros((0, 256))


@pytest.mark.parametrize("n,gap", [(257, None), (384, None), (385, None), (513, None), (4224, None), (4225, None),
                                   (4352, None), (20000, (3000, 9000)), (20000, (0, 4000)), (20000, (15000, 20000))])
def test_reframing_mirror_matches_silent_frame_removal(n, gap):
    """Kept-frame count K, re-framed count K - 1 and every re-framed, twice-windowed frame against the host's route through
    an intermediate signal -- on lengths around 30 and 31 kept frames (4224, 4225: 31 frames; 4352: 32) and with silent
    spans at the start, in the middle and at the end."""
    from aware_amd import runtime as rt
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n)
    if gap:
        x[gap[0]:gap[1]] *= 1e-4
    w = np.hanning(258)[1:-1]
    xf = M._frames(x, 256, 128, w)
    assert len(xf) == rt.stoi_frames(n)
    if len(xf):
        e = 20 * np.log10(np.linalg.norm(xf, axis=1) + M._EPS)
        kept = np.nonzero((np.max(e) - 40.0 - e) < 0)[0]
    else:
        kept = np.zeros(0, dtype=int)
    xs, _ = M._remove_silent_frames(x, x, 40.0, 256, 128)
    host_rows = M._frames(xs, 256, 128, w)
    assert len(host_rows) == rt.stoi_reframed(len(kept))
    mirror = _reframe_mirror(x, kept, w)
    assert mirror.shape == host_rows.shape
    np.testing.assert_allclose(mirror, host_rows, rtol=0, atol=1e-14)
    assert rt.stoi_segments(len(kept)) == max(len(host_rows) - 29, 0)


@pytest.mark.parametrize("kept,segments", [(0, 0), (1, 0), (2, 0), (30, 0), (31, 1), (32, 2), (100, 70)])
def test_segment_count(kept, segments):
    """30 re-framed frames are the fewest that give a segment, i.e. 31 kept frames; below that the score is 1e-5."""
    from aware_amd import runtime as rt
    assert rt.stoi_segments(kept) == segments
    x = np.random.default_rng(kept).standard_normal(128 * kept + 129 if kept else 200)     # all frames kept (white noise)
    assert rt.stoi_frames(len(x)) == kept
    s = M.stoi(x, x, 10000)
    assert (s == 1e-5) == (segments == 0)


def test_band_edges_are_the_host_matrix(lib):
    obm = M._third_octave_matrix(10000, 512, 15, 150.0)
    lo, hi = (C.c_int * 15)(), (C.c_int * 15)()
    assert lib.aware_stoi_band_edges(None, lo, hi) == 0
    mine = np.zeros_like(obm)
    for k in range(15):
        assert 0 <= lo[k] < hi[k] <= 256                      # the kernel's band sums read bins 0..255
        mine[k, lo[k]:hi[k]] = 1.0
    np.testing.assert_array_equal(mine, obm)
    assert lib.aware_stoi_band_edges(None, None, hi) == -1


def test_workspace_grows_and_covers_every_frame_kept(lib):
    from aware_amd import runtime as rt
    ws = lib.aware_stoi_workspace_bytes

    def need(lengths):
        tf = sum(rt.stoi_frames(n) for n in lengths)
        nseg = max(rt.stoi_segments(rt.stoi_frames(max(lengths))), 1)
        return tf * (8 + 4 + 2 * 16 * 4) + len(lengths) * (4 + 4) + len(lengths) * -(-nseg // 64) * 8

    for lengths in ([30000], [30000] * 4, [30000] * 256, [10000, 100000, 600000], [257] * 7, [100] * 3, [1875000, 257]):
        assert ws(len(lengths), max(lengths), sum(lengths)) >= need(lengths), lengths
    assert ws(1, 30000, 30000) < ws(2, 30000, 60000) < ws(64, 30000, 64 * 30000) < ws(256, 30000, 256 * 30000)
    assert ws(4, 30000, 120000) < ws(4, 100000, 400000)
    # a ragged batch with one long clip is sized by the total, not by B x the longest clip
    assert ws(256, 1875000, 1875000 + 255 * 30000) < ws(256, 1875000, 256 * 1875000) / 20
    assert ws(0, 30000, 30000) == 0 and ws(1, -1, 0) == 0


def test_null_arguments_are_refused_before_any_device_work(lib):
    assert lib.aware_stoi(None, None, None, None, None, None, 1, 1000, 1000, None, None, None, 0, None) == -1
    assert lib.aware_stoi_create(None) == -1
    lib.aware_stoi_destroy(None)                              # a no-op, as for the other handles


@pytest.mark.parametrize("sr", [16000, 20000, 44100, 8000])
def test_resampling_filter_is_what_the_host_hands_to_scipy(sr):
    """_resample_oct calls resample_poly(x, up, down, window=h / sum(h)), which scales the taps by `up` and aligns the output
    so that y[j] = sum_i x[i] h[j down - i up + half]: the device's taps in float32, and that formula against scipy."""
    from scipy.signal import resample_poly
    from aware_amd import runtime as rt
    h, up, down, half = rt.stoi_resample_filter(sr)
    g = np.gcd(10000, sr)
    assert (up, down) == (10000 // g, sr // g) and h.dtype == np.float32 and len(h) == 2 * half + 1
    ref = M._resample_window_oct(10000, sr)
    ref = ref / np.sum(ref) * up
    np.testing.assert_array_equal(h, ref.astype(np.float32))
    x = np.random.default_rng(sr).standard_normal(300)
    want = M._resample_oct(x, 10000, sr)
    assert len(want) == -(-len(x) * up // down)
    got = np.zeros(len(want))
    for j in range(len(want)):
        for i in range(len(x)):
            t = j * down - i * up + half
            if 0 <= t < len(ref):
                got[j] += x[i] * ref[t]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
