"""Shift search in detection (EXTENSION): the grid and its validation (aware_amd/detection/sync.py::check_shift_search,
shift_offsets, shift_of), the views and their refusals, the selection's tie rule, the detector's and the service's keys, the
card key, the C ABI's symbol and refusals, and the value claim on the CPU -- a clip whose every component was moved by the
same number of Hz reads its bits again once the detector looks at 31 candidate shifts.  No GPU."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, make_clip
from oracle import aware_oracle as O
from aware_amd.detection import sync as S
from aware_amd.embedding import loop_attacks as LA

GRID = {"max_hz": 150, "step_hz": 10}
SHIFTS_HZ = [20.0, -33.0, 50.0, -77.0, 100.0, 123.4]       # the received shifts of the value claim


# ---- 1. the grid and its validation -------------------------------------------------------------------------------------------------
def test_the_grid():
    assert S.SHIFT_MAX_VIEWS == 63 and S.SHIFT_STEP_DEFAULT == 10.0
    ds = S.shift_offsets(GRID, 16000)
    assert LA.shift_increment(10, 16000) == 655 and LA.shift_increment(10, 44100) == 238
    assert len(ds) == 31 and ds[:5] == [0, -655, 655, -1310, 1310] and ds[-2:] == [-9825, 9825]
    assert ds == [0] + [s * i * 655 for i in range(1, 16) for s in (-1, 1)]
    assert [abs(d) for d in ds] == sorted(abs(d) for d in ds)                              # ordered by |d|: ties prefer the plain read
    assert S.shift_offsets(GRID, 44100)[:3] == [0, -238, 238] and len(S.shift_offsets(GRID, 44100)) == 31
    assert S.check_shift_search(GRID) == {"max_hz": 150.0, "step_hz": 10.0}
    # a number is max_hz at step 10
    for v in (150, 150.0, np.float32(150.0), np.int64(150)):
        assert S.check_shift_search(v) == {"max_hz": 150.0, "step_hz": 10.0} and S.shift_offsets(v, 16000) == ds
    assert S.check_shift_search({"max_hz": 40}) == {"max_hz": 40.0, "step_hz": 10.0}
    assert S.shift_offsets({"max_hz": 45, "step_hz": 20}, 16000) == [0, -1311, 1311, -2622, 2622]           # K = floor(2.25)
    assert S.shift_offsets({"max_hz": 3.0, "step_hz": 1.0}, 16000) == [0, -66, 66, -132, 132, -198, 198]     # K = floor(3 + 1e-9)
    assert S.shift_offsets(10, 16000) == [0, -655, 655] and S.shift_offsets({"max_hz": 19.9}, 16000) == [0, -655, 655]
    # the 63-view cap: 310 Hz every 10 Hz is 63 views, 320 Hz is 65
    assert len(S.shift_offsets(310, 16000)) == 63 and len(S.shift_offsets({"max_hz": 31, "step_hz": 1}, 16000)) == 63
    with pytest.raises(ValueError, match="63"):
        S.check_shift_search(320)
    with pytest.raises(ValueError, match="63"):
        S.check_shift_search({"max_hz": 32, "step_hz": 1})
    # max_hz may not exceed sample_rate / 16, the operator's range: 16 kHz allows 1000 Hz, 8 kHz 500 Hz
    assert max(S.shift_offsets({"max_hz": 600, "step_hz": 20}, 16000)) == 30 * 1311 <= LA.MAX_SHIFT
    assert max(S.shift_offsets({"max_hz": 500, "step_hz": 20}, 8000)) == 25 * 2621 <= LA.MAX_SHIFT
    with pytest.raises(ValueError, match="500"):
        S.shift_offsets({"max_hz": 520, "step_hz": 20}, 8000)                              # 26 x 2621 = 68146 > 65536
    with pytest.raises(ValueError):
        S.shift_offsets({"max_hz": 300, "step_hz": 10}, 4000)                              # sr / 16 = 250 Hz


def test_shift_of_is_the_sign_inverse_of_shift_increment():
    for sr in (16000, 44100, 8000):
        for hz in (10.0, -33.0, 123.4, 250.0):
            d = LA.shift_increment(hz, sr)
            assert S.shift_of(d, sr) == pytest.approx(-hz, abs=0.5 * sr / 2 ** 20 + 1e-9)  # the view at d undoes a shift of -hz
            assert LA.shift_increment(-S.shift_of(d, sr), sr) == d
    assert S.shift_of(0, 16000) == 0.0 and S.shift_of(-655, 16000) == pytest.approx(9.9945, abs=1e-4)
    assert S.shift_of(1 << 16, 16000) == -1000.0


@pytest.mark.parametrize("off", [None, 0, 0.0, False, {}])
def test_off_values(off):
    assert S.check_shift_search(off) is None and S.shift_offsets(off, 16000) == [0]
    assert S.shift_views([16000, 600], off, 16000) == [16000, 600]


@pytest.mark.parametrize("bad", [
    float("nan"), float("inf"), {"max_hz": float("nan")}, {"max_hz": 150, "step_hz": float("inf")},                    # not finite
    {"max_hz": 150, "step_hz": 0.5}, {"max_hz": 150, "step_hz": 20.5}, {"max_hz": 150, "step_hz": 0},                  # the step's range
    5, -50, {"max_hz": 10, "step_hz": 15},                                                                              # max_hz below the step
    {"max_hz": 150, "step": 10}, {"max_hz": 150, "step_hz": 10, "refine": True}, {"step_hz": 10}, {"max_percent": 12}, # keys
    320, {"max_hz": 150, "step_hz": 2}, {"max_hz": 1000, "step_hz": 20},                                              # more than 63 views
    True, "150", [150, 10], {"max_hz": "150"}, {"max_hz": 150, "step_hz": None}])                                     # not numbers
def test_bad_shift_search_is_refused(bad):
    with pytest.raises(ValueError, match="shift_search"):
        S.check_shift_search(bad)
    from aware_amd.detection import AWAREDetector
    with pytest.raises(ValueError):
        AWAREDetector(model=None, shift_search=bad)


def test_the_detector_keys_and_refusals():
    from aware_amd.detection import AWAREDetector
    det = AWAREDetector(model=None)
    assert det.shift_search is None and det.speed_search is None and det.sync_search == 0
    assert AWAREDetector(model=None, shift_search=150).shift_search == {"max_hz": 150.0, "step_hz": 10.0}
    assert AWAREDetector(model=None, shift_search=0).shift_search is None
    assert inspect.signature(AWAREDetector.__init__).parameters["shift_search"].default is None
    sig = inspect.signature(det.detect_batch_shift).parameters
    assert list(sig) == ["clips", "sample_rate", "shift_search", "sync_search", "return_shift"]
    assert sig["shift_search"].default is None and sig["sync_search"].default is None and sig["return_shift"].default is False
    # not together with the speed search, at construction and per call; both before any plan or launch (model=None)
    with pytest.raises(ValueError, match="speed_search and shift_search"):
        AWAREDetector(model=None, shift_search=150, speed_search=12.0)
    clip = [np.zeros(16000, dtype=np.float32)]
    with pytest.raises(ValueError, match="speed_search and shift_search"):
        AWAREDetector(model=None, speed_search=12.0).detect_batch_shift(clip, 16000, shift_search=150)
    with pytest.raises(ValueError, match="speed_search and shift_search"):
        AWAREDetector(model=None, shift_search=150).detect_batch(clip, 16000, speed_search=12.0)
    # scan on a detector that searches shifts
    with pytest.raises(ValueError, match="scan: shift_search"):
        AWAREDetector(model=None, shift_search=150).scan(clip, 16000)
    # the general route does not serve it, at construction and per call
    geom = dict(frame_length=512, hop_length=128, win_length=512, general_geometry=True)
    with pytest.raises(NotImplementedError, match="shift_search"):
        AWAREDetector(model=None, shift_search=150, **geom)
    with pytest.raises(NotImplementedError, match="shift_search"):
        AWAREDetector(model=None, **geom).detect_batch_shift(clip, 16000, shift_search=150)
    # a grid past sample_rate / 16 and a clip too short, by its index
    with pytest.raises(ValueError, match="shift_search"):
        det.detect_batch_shift(clip, 4000, shift_search=300)
    with pytest.raises(ValueError, match="clip 1"):
        det.detect_batch_shift(clip + [np.zeros(512, dtype=np.float32)], 16000, shift_search=150)
    with pytest.raises(ValueError, match="clip 0"):
        det.detect_batch_shift([np.zeros(960, dtype=np.float32)], 16000, shift_search=150, sync_search=8)


# ---- 2. the views and the selection -----------------------------------------------------------------------------------------------
def test_view_lengths_and_refusals():
    lengths = [16000, 1000, 4099]
    v = S.shift_views(lengths, GRID, 16000)
    assert v == [n for n in lengths for _ in range(31)]                                    # every view has the clip's length
    assert S.shift_views(lengths, GRID, 16000, 8) == v
    S.shift_views([513], GRID, 16000)
    with pytest.raises(ValueError, match="clip 0"):
        S.shift_views([512], GRID, 16000)
    with pytest.raises(ValueError, match="clip 1"):
        S.shift_views([16000, 300], 150, 16000)
    # with the offset search the largest offset, 448 of sync_search = 8, comes off every view
    S.shift_views([16000, 961], GRID, 16000, 8)
    with pytest.raises(ValueError, match="clip 1.*sync_search = 8"):
        S.shift_views([16000, 960], GRID, 16000, 8)
    with pytest.raises(ValueError, match="clip 2"):
        S.shift_views([16000, 16000, 1016], 150, 16000, 64)
    # the views of one clip together: 31 views of 2^26 samples are more than 2^30
    with pytest.raises(ValueError, match="clip 1.*2\\^30"):
        S.shift_views([16000, 1 << 26], GRID, 16000)
    S.shift_views([1 << 24], GRID, 16000)
    with pytest.raises(ValueError):
        S.shift_views([16000], {"max_hz": 150, "step_hz": 0.1}, 16000)


@pytest.mark.parametrize("n_shift, n_sync", [(31, 0), (31, 8), (63, 2), (3, 0)])
def test_shift_select_is_speed_select_and_prefers_the_plain_read_on_a_tie(n_shift, n_sync):
    rows, L, B = n_shift * max(n_sync, 1), 20, 3
    rng = np.random.default_rng(n_shift + n_sync)
    v = (0.2 * rng.uniform(0.5, 0.9, size=(B * rows, L)) * rng.choice([-1.0, 1.0], size=(B * rows, L))).astype(np.float32)
    win = rng.integers(1, rows, size=B)
    first = []
    for b in range(B):                                                                     # a clear winner, and its row once more
        v[b * rows + win[b]] *= np.float32(2.0)
        j = (int(win[b]) + 1 + 3 * b) % rows
        v[b * rows + j] = v[b * rows + win[b]]
        first.append(min(int(win[b]), j))
    out, idx, conf = S.shift_select(v, n_shift, n_sync, 0.0)
    ref = S.speed_select(v, n_shift, n_sync, 0.0)
    assert idx.tolist() == first and idx.dtype == np.int32 and conf.dtype == np.float32 and out.shape == (B, L)
    for a, b in zip((out, idx, conf), ref):
        np.testing.assert_array_equal(a, b)
    same = np.tile(v[:1], (2 * rows, 1))                                                   # all rows equal: the plain read, d = 0
    assert S.shift_select(same, n_shift, n_sync)[1].tolist() == [0, 0]


# ---- 3. the service, the card, the ABI ----------------------------------------------------------------------------------------------
def test_the_service_follows_the_detector():
    from aware_amd.service.detect import detect_watermark, detect_watermark_batch

    class Shifting:
        pattern_mode, threshold = "bits2bipolar", 0.0
        sync_search, speed_search, shift_search = 0, None, None
        calls = []

        def detect(self, audio, sr):
            return np.array([0.5, -0.5], dtype=np.float32)

        def detect_batch(self, clips, sr, sync_search=None, return_sync=False, speed_search=None, return_speed=False):
            self.calls.append(("batch", sync_search, return_sync, speed_search, return_speed))
            v, z = torch.tensor([[0.5, -0.5]] * len(clips)), torch.zeros(len(clips), dtype=torch.int32)
            return (v, z, z, torch.ones(len(clips))) if return_speed else ((v, z, torch.ones(len(clips))) if return_sync else v)

        def detect_batch_shift(self, clips, sr, shift_search=None, sync_search=None, return_shift=False):
            self.calls.append(("shift", shift_search, sync_search, return_shift))
            v, z = torch.tensor([[0.5, -0.5]] * len(clips)), torch.zeros(len(clips), dtype=torch.int32)
            return (v, z, z, torch.ones(len(clips))) if return_shift else v

    a = np.zeros(2000, dtype=np.float32)
    p = Shifting()
    want = list(detect_watermark(a, 16000, p))
    assert p.calls == []                                                                   # every search off: detect(), plainly
    assert [list(b) for b in detect_watermark_batch([a], 16000, p)] == [want] and p.calls[-1] == ("batch", None, False, None, False)
    p.shift_search = {"max_hz": 150.0, "step_hz": 10.0}                                    # the detector's own
    assert list(detect_watermark(a, 16000, p)) == want and p.calls[-1] == ("shift", None, None, True)
    assert list(detect_watermark(np.stack([a, a], axis=1), 16000, p, sync_search=8)) == want and p.calls[-1] == ("shift", None, 8, True)
    assert [list(b) for b in detect_watermark_batch([a, a], 16000, p)] == [want, want] and p.calls[-1] == ("shift", None, None, True)
    # a speed search asked for on top goes to detect_batch, which refuses the pair
    detect_watermark(a, 16000, p, speed_search=12.0)
    assert p.calls[-1] == ("batch", None, False, 12.0, True)


def test_card_key_reaches_the_detector(tmp_path):
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        text = f.read()
    assert "# shift_search: {max_hz: 150.0, step_hz: 10.0}" in text
    card = yaml.safe_load(text)
    assert "shift_search" not in card
    assert load()[1].shift_search is None                                                  # the committed card keeps its behaviour
    p = tmp_path / "card.yaml"
    for value, want in (({"max_hz": 150.0, "step_hz": 10.0}, {"max_hz": 150.0, "step_hz": 10.0}),
                        (100, {"max_hz": 100.0, "step_hz": 10.0}), (0, None)):
        card["shift_search"] = value
        p.write_text(yaml.safe_dump(card))
        det = load(str(p))[1]
        assert det.shift_search == want and det.sync_search == 0 and det.speed_search is None
    for bad in ({"max_hz": 150.0, "step_hz": 2.0}, 400, {"hz": 150}):
        card["shift_search"] = bad
        p.write_text(yaml.safe_dump(card))
        assert load(str(p)) is None
    card["shift_search"], card["speed_search"] = 150, 12.0                                 # the pair is refused at construction
    p.write_text(yaml.safe_dump(card))
    assert load(str(p)) is None
    card["shift_search"], card["speed_search"], card["general_geometry"] = 150, 0, True
    p.write_text(yaml.safe_dump(card))
    assert load(str(p)) is None


def test_abi_symbol_and_bad_arguments():
    from aware_amd import _lib
    lib = _lib.load_library()
    assert "aware_shift_views" in _lib.SIGNATURES and hasattr(lib, "aware_shift_views")
    assert "shift_search_kernels.hip" in _lib.SOURCES and len(_lib.SIGNATURES["aware_shift_views"][1]) == 10
    assert lib.aware_version() == 350                                                      # added without a version step
    with open(os.path.join(ROOT, "include", "aware_hip.h")) as f:
        assert ("int aware_shift_views(const float* in, const int* in_off, const int* in_len, int B, const int* d, int n_views, "
                "float* out,") in f.read()
    for name in ("kernels.h", "capi.hip"):
        with open(os.path.join(ROOT, "aware_amd", "csrc", name)) as f:
            assert "_shift_views(const float* in, const int* in_off, const int* in_len, int B, const int* d, int n_views" in f.read()
    # the Hilbert transformer's tile body is one header for both kernels
    for name in ("loop_shift_kernels.hip", "shift_search_kernels.hip"):
        with open(os.path.join(ROOT, "aware_amd", "csrc", name)) as f:
            src = f.read()
        assert '#include "shift_hilbert.hpp"' in src and "acc[m] += h * w[m]" not in src
    assert lib.aware_shift_views(None, None, None, 1, None, 31, None, None, 16000, None) == -1
    p, q = C.c_void_p(256), C.c_void_p(512)                 # never dereferenced: every call below is refused
    for i in range(6):                                      # each pointer in turn
        a = [p, p, p, p, q, p]
        a[i] = None
        assert lib.aware_shift_views(a[0], a[1], a[2], 1, a[3], 31, a[4], a[5], 16000, None) == -1, i
    for B, nv, max_len in ((0, 31, 16000), (-1, 31, 16000), (65536, 31, 16000), (1, 0, 16000), (1, 64, 16000), (1, -3, 16000),
                           (1, 31, 0), (1, 31, -5), (1, 31, (1 << 30) + 1)):
        assert lib.aware_shift_views(p, p, p, B, p, nv, q, p, max_len, None) == -1, (B, nv, max_len)
    assert lib.aware_shift_views(p, p, p, 1, p, 31, p, p, 16000, None) == -1               # in == out


# ---- 4. the value claim, on the CPU ---------------------------------------------------------------------------------------------
def ssb(y, hz, sr=16000):
    """Re(analytic(y) e^{j 2 pi hz t}) with the FFT analytic signal: a construction independent of the views' FIR."""
    n = y.shape[-1]
    spec = np.fft.fft(y.astype(np.float64), axis=-1)
    gain = np.zeros(n)
    gain[0] = 1.0
    gain[1:(n + 1) // 2] = 2.0
    if n % 2 == 0:
        gain[n // 2] = 1.0
    analytic = np.fft.ifft(spec * gain, axis=-1)
    return np.real(analytic * np.exp(2j * np.pi * hz * np.arange(n) / sr)).astype(np.float32)


def best_views(plain, z, ds):
    """z [B, n] -> shift_select over the views of the oracle's detector: (values, index, confidence, the plain read)."""
    zt = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32))
    rows = [plain.detect_raw(np.ascontiguousarray(LA.frequency_shift(zt, d, 0).numpy())).numpy() for d in ds]
    v = np.stack(rows, axis=1)                                                             # [B, n_shift, 20]
    out, idx, conf = S.shift_select(v.reshape(-1, v.shape[-1]), len(ds), 0, 0.0)
    return out, idx, conf, v[:, 0]


@pytest.fixture(scope="module")
def marked():
    """Four 1 s clips embedded plainly by the CPU oracle, 400 steps, once for the module."""
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    pairs = [make_clip(s, 16000) for s in range(4)]
    audio = np.stack([p[0] for p in pairs])
    bits = np.stack([p[1] for p in pairs])
    wm = np.stack([O.bits_to_bipolar(b) for b in bits]).astype(np.float32)
    plain = O.Embedder()
    y = plain.embed(audio, wm)[0].numpy()
    return plain, audio, y, bits


def test_the_search_recovers_shifted_clips(marked):
    """Received shifts of +20, -33, +50, -77, +100 and +123.4 Hz: the plain read loses at least a quarter of the bits on
    average (measured 47.1 %), the best of the 31 views of {"max_hz": 150, "step_hz": 10} loses none, the chosen view undoes
    the shift to within one grid step, and its confidence is at least 0.12 (the smallest measured in this range: 0.162)."""
    plain, audio, y, bits = marked
    ds = S.shift_offsets(GRID, 16000)
    assert len(ds) == 31
    out, idx, conf, _ = best_views(plain, y, ds)
    print(f"no shift: chosen d {[ds[j] for j in idx]}, confidence {[round(float(c), 3) for c in conf]}")
    assert float((O.decode_bits(out) != bits).mean()) == 0.0 and idx.tolist() == [0] * 4   # clean: the plain read, every bit
    plain_ber = []
    for hz in SHIFTS_HZ:
        z = ssb(y, hz)
        out, idx, conf, first = best_views(plain, z, ds)
        b0 = 100.0 * float((O.decode_bits(first) != bits).mean())
        b1 = 100.0 * float((O.decode_bits(out) != bits).mean())
        found = [S.shift_of(ds[j], 16000) for j in idx]
        print(f"{hz:+.1f} Hz: plain {b0:.2f} % / best of 31 views {b1:.2f} %; found {[round(f, 1) for f in found]} Hz, "
              f"confidence {[round(float(c), 3) for c in conf]}")
        plain_ber.append(b0)
        assert b1 == 0.0, hz
        # shift_of(d) is the shift the clip carried when the view at d restores it: within one grid step of the truth
        assert max(abs(f - hz) for f in found) <= 10.0, (hz, found)
        assert float(conf.min()) >= 0.12, (hz, conf)
    print(f"plain mean BER {np.mean(plain_ber):.2f} %")
    assert float(np.mean(plain_ber)) >= 25.0, plain_ber


def test_unmarked_audio_stays_below_the_scan_threshold(marked):
    """The largest confidence of unmarked audio over the 63 views of +-310 Hz stays below SCAN_MIN_CONFIDENCE (measured 0.026)."""
    plain, audio, y, bits = marked
    ds = S.shift_offsets(310, 16000)
    assert len(ds) == 63
    _, _, conf, first = best_views(plain, audio[:, :y.shape[1]], ds)
    print(f"unmarked hosts: largest confidence over the 63 views {[round(float(c), 4) for c in conf]}, "
          f"plain {[round(float(c), 4) for c in np.abs(first).mean(axis=1)]}")
    assert float(conf.max()) < S.SCAN_MIN_CONFIDENCE
