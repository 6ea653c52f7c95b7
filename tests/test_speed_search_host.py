"""Speed search in detection (EXTENSION): the grid and its validation (aware_amd/detection/sync.py::check_speed_search,
speed_offsets), the view lengths and their refusals, the selection's restatement against the flat argmax and against two
rounds of sync_select, the service's call pattern, the card key, the C ABI's symbol and refusals, and the value claim on the
CPU -- a clip that was played at another speed reads its bits again once the detector looks at 49 speeds.  No GPU."""
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

GRID = {"max_percent": 12, "step_percent": 0.5}
# the attacks of the value claim: resample_poly(up, down) plays the clip at down / up of its speed
RATIOS = [(20, 21), (20, 19), (10, 11), (10, 9), (100, 103), (100, 93), (400, 431)]


# ---- 1. the grid and its validation -------------------------------------------------------------------------------------------------
def test_the_grid():
    ms = S.speed_offsets(GRID)
    assert len(ms) == 49 and ms[0] == 0 and ms[1:5] == [-328, 328, -656, 656] and ms[-2:] == [-7872, 7872]
    assert ms == [0] + [s * i * 328 for i in range(1, 25) for s in (-1, 1)]
    assert [abs(m) for m in ms] == sorted(abs(m) for m in ms)                              # ordered by |m|: ties prefer the plain read
    assert min(ms) == -7872 and max(ms) == 7872
    assert S.check_speed_search(GRID) == {"max_percent": 12.0, "step_percent": 0.5}
    # a number is max_percent at step 0.5
    for v in (12, 12.0, np.float32(12.0), np.int64(12)):
        assert S.check_speed_search(v) == {"max_percent": 12.0, "step_percent": 0.5} and S.speed_offsets(v) == ms
    assert S.check_speed_search({"max_percent": 3}) == {"max_percent": 3.0, "step_percent": 0.5}
    assert S.speed_offsets({"max_percent": 3.0, "step_percent": 1.0}) == [0, -655, 655, -1310, 1310, -1965, 1965]
    assert S.speed_offsets({"max_percent": 0.3, "step_percent": 0.1}) == [0, -66, 66, -132, 132, -198, 198]      # K = floor(3 + 1e-9)
    assert len(S.speed_offsets({"max_percent": 15.5, "step_percent": 0.5})) == 63          # the most views there are
    assert len(S.speed_offsets({"max_percent": 20, "step_percent": 2})) == 21
    assert S.speed_of(0) == 1.0 and S.speed_of(-3121) == pytest.approx(1.05, abs=1e-4) and S.speed_of(7282) == pytest.approx(0.9, abs=1e-4)
    # the widest grids stay inside the operator's range of offsets, -13520..17034
    for g in ({"max_percent": 20, "step_percent": 0.65}, {"max_percent": 20, "step_percent": 2}, {"max_percent": 20, "step_percent": 1.0}):
        assert -13520 <= min(S.speed_offsets(g)) and max(S.speed_offsets(g)) <= 13500


@pytest.mark.parametrize("off", [None, 0, 0.0, False, {}])
def test_off_values(off):
    assert S.check_speed_search(off) is None and S.speed_offsets(off) == [0]


@pytest.mark.parametrize("bad", [
    float("nan"), float("inf"), {"max_percent": float("nan")}, {"max_percent": 12, "step_percent": float("inf")},       # not finite
    {"max_percent": 12, "step_percent": 0.04}, {"max_percent": 12, "step_percent": 2.5},                               # the step's range
    0.4, -5, {"max_percent": 0.5, "step_percent": 1.0}, 20.5, {"max_percent": 21, "step_percent": 2},                  # max's range
    {"max_percent": 12, "step": 0.5}, {"max_percent": 12, "step_percent": 0.5, "refine": True}, {"step_percent": 0.5},  # keys
    16.0, {"max_percent": 12, "step_percent": 0.25}, {"max_percent": 20, "step_percent": 0.5},                          # more than 63 views
    True, "12", [12, 0.5], {"max_percent": "12"}, {"max_percent": 12, "step_percent": None}])                          # not numbers
def test_bad_speed_search_is_refused(bad):
    with pytest.raises(ValueError):
        S.check_speed_search(bad)
    from aware_amd.detection import AWAREDetector
    with pytest.raises(ValueError):
        AWAREDetector(model=None, speed_search=bad)


def test_defaults_and_signatures():
    from aware_amd.detection import AWAREDetector
    from aware_amd.service import detect as SD
    det = AWAREDetector(model=None)
    assert det.speed_search is None and det.sync_search == 0
    assert AWAREDetector(model=None, speed_search=12.0).speed_search == {"max_percent": 12.0, "step_percent": 0.5}
    assert AWAREDetector(model=None, speed_search=0).speed_search is None
    sig = inspect.signature(det.detect_batch).parameters
    assert list(sig) == ["clips", "sample_rate", "sync_search", "return_sync", "speed_search", "return_speed"]
    assert sig["speed_search"].default is None and sig["return_speed"].default is False
    assert sig["sync_search"].default is None and sig["return_sync"].default is False
    assert list(inspect.signature(det.detect).parameters) == ["audio", "sample_rate", "sync_search", "speed_search"]
    assert inspect.signature(det.detect).parameters["speed_search"].default is None
    for fn in (SD.detect_watermark, SD.detect_watermark_batch):
        assert list(inspect.signature(fn).parameters)[-2:] == ["sync_search", "speed_search"]
        assert inspect.signature(fn).parameters["speed_search"].default is None


# ---- 2. the views --------------------------------------------------------------------------------------------------------------------
def test_view_lengths_and_refusals():
    ms = S.speed_offsets(GRID)
    lengths = [16000, 1000, 4099]
    v = S.speed_views(lengths, GRID)
    assert v == [LA.speed_length(n, m) for n in lengths for m in ms]
    assert v[:3] == [16000, 16080, 15920] and len(v) == 3 * 49
    assert S.speed_views([16000, 4099], GRID, 8) == v[:49] + v[98:]                        # the lengths are those of the speed views
    for n, m in ((16000, 7872), (16000, -7872), (5, 328), (1, 7872)):                      # every position lies inside the clip
        assert (LA.speed_length(n, m) - 1) * (65536 + m) <= (n - 1) << 16 < LA.speed_length(n, m) * (65536 + m)
    # the shortest view of n samples at +12 % is ((n - 1) << 16) // 73408 + 1: 574 samples give 512, 575 give 513
    assert LA.speed_length(574, 7872) == 512 and LA.speed_length(575, 7872) == 513
    S.speed_views([575], GRID)
    with pytest.raises(ValueError, match="clip 0"):
        S.speed_views([574], GRID)
    with pytest.raises(ValueError, match="clip 1"):
        S.speed_views([16000, 520], 12.0)
    # with the offset search the largest offset comes off the shortest view: 900 samples at +12 % are 803, less 448 are 355
    assert LA.speed_length(900, 7872) == 803
    S.speed_views([16000, 900], GRID)
    with pytest.raises(ValueError, match="clip 1"):
        S.speed_views([16000, 900], GRID, 8)
    with pytest.raises(ValueError, match="clip 2"):
        S.speed_views([16000, 16000, 900], 12.0, 64)
    S.speed_views([1077], GRID, 8)                                                         # 961 samples at +12 %, less 448: 513
    with pytest.raises(ValueError):
        S.speed_views([1075], GRID, 8)
    # the views of one clip together: 49 views of 2^25 samples are more than 2^30
    with pytest.raises(ValueError, match="clip 1.*2\\^30"):
        S.speed_views([16000, 1 << 25], GRID)
    S.speed_views([1 << 24], 3.0)
    with pytest.raises(ValueError):
        S.speed_views([16000], {"max_percent": 12, "step_percent": 0.01})


# ---- 3. the selection ----------------------------------------------------------------------------------------------------------------
def two_rounds(v, n_speed, n_sync, centre):
    """Round one over the sync views of every (clip, speed view), round two over the speed views: how the device selects."""
    if n_sync:
        v1, i1, _ = S.sync_select(v, n_sync, centre)
    else:
        v1, i1 = v, np.zeros(len(v), dtype=np.int32)
    out, i2, conf = S.sync_select(v1, n_speed, centre)
    B = len(out)
    flat = i2 * max(n_sync, 1) + i1.reshape(B, n_speed)[np.arange(B), i2]
    return out, flat.astype(np.int32), conf


def clear_winners(B, rows, L, seed, centre):
    """Random rows around `centre` with one clear winner per clip: scaled by 2, its confidence is more than a tenth above every other."""
    rng = np.random.default_rng(seed)
    v = (centre + 0.2 * rng.uniform(0.5, 0.9, size=(B * rows, L)) * rng.choice([-1.0, 1.0], size=(B * rows, L))).astype(np.float32)
    win = rng.integers(0, rows, size=B)
    for b in range(B):
        v[b * rows + win[b]] = (centre + 2.0 * (v[b * rows + win[b]] - centre)).astype(np.float32)
    return v, win.astype(np.int32)


@pytest.mark.parametrize("n_speed, n_sync", [(49, 0), (49, 8), (3, 64), (63, 2), (1, 4), (7, 0)])
@pytest.mark.parametrize("centre", [0.0, 0.5])
def test_speed_select_is_the_flat_argmax_and_two_rounds(n_speed, n_sync, centre):
    rows, L, B = n_speed * max(n_sync, 1), 20, 3
    v, win = clear_winners(B, rows, L, 7 * n_speed + n_sync, centre)
    conf64 = np.abs(v.astype(np.float64) - centre).mean(axis=1).reshape(B, rows)
    top = np.sort(conf64, axis=1)[:, ::-1]
    assert np.all(top[:, 1] < 0.99 * top[:, 0])                                            # the order of a float32 sum decides nothing
    out, idx, conf = S.speed_select(v, n_speed, n_sync, centre)
    assert out.dtype == np.float32 and out.shape == (B, L) and idx.dtype == np.int32 and conf.dtype == np.float32
    np.testing.assert_array_equal(idx, win)
    np.testing.assert_array_equal(idx, np.argmax(conf64, axis=1))
    np.testing.assert_array_equal(out.view(np.uint32), v.reshape(B, rows, L)[np.arange(B), win].view(np.uint32))
    o2, i2, c2 = two_rounds(v, n_speed, n_sync, centre)
    np.testing.assert_array_equal(i2, idx)
    np.testing.assert_array_equal(o2.view(np.uint32), out.view(np.uint32))
    np.testing.assert_array_equal(c2.view(np.uint32), conf.view(np.uint32))


@pytest.mark.parametrize("n_speed, n_sync", [(49, 0), (49, 8), (5, 4)])
def test_speed_select_ties(n_speed, n_sync):
    rows, L, B = n_speed * max(n_sync, 1), 20, 3
    v, win = clear_winners(B, rows, L, n_speed + n_sync, 0.0)
    first = win.copy()
    for b in range(B):                                                                     # the winner's row once more, elsewhere
        j = (int(win[b]) + 1 + 3 * b) % rows
        v[b * rows + j] = v[b * rows + win[b]]
        first[b] = min(int(win[b]), j)
    out, idx, conf = S.speed_select(v, n_speed, n_sync, 0.0)
    np.testing.assert_array_equal(idx, first)
    o2, i2, c2 = two_rounds(v, n_speed, n_sync, 0.0)
    np.testing.assert_array_equal(i2, first)
    np.testing.assert_array_equal(c2.view(np.uint32), conf.view(np.uint32))
    same = np.tile(v[:1], (2 * rows, 1))                                                   # all rows equal: the plain read
    assert S.speed_select(same, n_speed, n_sync)[1].tolist() == [0, 0] and two_rounds(same, n_speed, n_sync, 0.0)[1].tolist() == [0, 0]
    with pytest.raises(ValueError):
        S.speed_select(v[:-1], n_speed, n_sync)


# ---- 4. the service, the card, the ABI ----------------------------------------------------------------------------------------------
def test_the_service_passes_the_keyword_only_where_it_is_asked_for():
    from aware_amd.service.detect import detect_watermark, detect_watermark_batch

    class Plain:
        pattern_mode, threshold = "bits2bipolar", 0.0

        def detect(self, audio, sr):
            return np.array([0.5, -0.5], dtype=np.float32)

        def detect_batch(self, clips, sr):
            return torch.tensor([[0.5, -0.5]] * len(clips))

    class Searching(Plain):                                 # knows the offset search only
        sync_search = 8
        calls = []

        def detect_batch(self, clips, sr, sync_search=None, return_sync=False):
            self.calls.append((sync_search, return_sync))
            v = torch.tensor([[0.5, -0.5]] * len(clips))
            return (v, torch.zeros(len(clips), dtype=torch.int32), torch.ones(len(clips))) if return_sync else v

    class Speeding(Plain):
        sync_search, speed_search = 0, None
        calls = []

        def detect_batch(self, clips, sr, sync_search=None, return_sync=False, speed_search=None, return_speed=False):
            self.calls.append((sync_search, return_sync, speed_search, return_speed))
            v, z = torch.tensor([[0.5, -0.5]] * len(clips)), torch.zeros(len(clips), dtype=torch.int32)
            return (v, z, z, torch.ones(len(clips))) if return_speed else ((v, z, torch.ones(len(clips))) if return_sync else v)

    a = np.zeros(2000, dtype=np.float32)
    want = list(detect_watermark(a, 16000, Plain()))
    assert list(detect_watermark(np.stack([a, a], axis=1), 16000, Plain())) == want
    assert [list(b) for b in detect_watermark_batch([a, a], 16000, Plain())] == [want, want]
    s = Searching()                                                                        # exactly as before
    assert list(detect_watermark(a, 16000, s)) == want and s.calls[-1] == (None, True)
    assert list(detect_watermark(a, 16000, s, sync_search=4)) == want and s.calls[-1] == (4, True)
    assert [list(b) for b in detect_watermark_batch([a], 16000, s, sync_search=0)] == [want] and s.calls[-1] == (0, True)
    p = Speeding()
    assert list(detect_watermark(a, 16000, p)) == want and p.calls == []                   # both searches off: detect(), plainly
    assert [list(b) for b in detect_watermark_batch([a], 16000, p)] == [want] and p.calls[-1] == (None, False, None, False)
    assert list(detect_watermark(a, 16000, p, sync_search=8)) == want and p.calls[-1] == (8, True, None, False)
    assert list(detect_watermark(a, 16000, p, speed_search=12.0)) == want and p.calls[-1] == (None, False, 12.0, True)
    assert list(detect_watermark(np.stack([a, a], axis=1), 16000, p, sync_search=8, speed_search=GRID)) == want
    assert p.calls[-1] == (8, False, GRID, True)
    assert [list(b) for b in detect_watermark_batch([a, a], 16000, p, speed_search=0)] == [want, want] and p.calls[-1] == (None, False, 0, True)
    p.speed_search = {"max_percent": 12.0, "step_percent": 0.5}                            # the detector's own
    assert list(detect_watermark(a, 16000, p)) == want and p.calls[-1] == (None, False, None, True)


def test_card_key_reaches_the_detector(tmp_path):
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        text = f.read()
    assert "# speed_search: {max_percent: 12.0, step_percent: 0.5}" in text
    card = yaml.safe_load(text)
    assert "speed_search" not in card
    assert load()[1].speed_search is None                                                  # the committed card keeps its behaviour
    p = tmp_path / "card.yaml"
    for value, want in (({"max_percent": 12.0, "step_percent": 0.5}, {"max_percent": 12.0, "step_percent": 0.5}),
                        (6, {"max_percent": 6.0, "step_percent": 0.5}), (0, None)):
        card["speed_search"] = value
        p.write_text(yaml.safe_dump(card))
        det = load(str(p))[1]
        assert det.speed_search == want and det.sync_search == 0
    card["sync_search"] = 8
    p.write_text(yaml.safe_dump(card))
    assert load(str(p))[1].sync_search == 8
    for bad in ({"max_percent": 12.0, "step_percent": 0.25}, 25, {"percent": 12}):
        card["speed_search"] = bad
        p.write_text(yaml.safe_dump(card))
        assert load(str(p)) is None


def test_abi_symbol_and_bad_arguments():
    from aware_amd import _lib
    lib = _lib.load_library()
    assert "aware_speed_views" in _lib.SIGNATURES and hasattr(lib, "aware_speed_views")
    assert "speed_search_kernels.hip" in _lib.SOURCES and len(_lib.SIGNATURES["aware_speed_views"][1]) == 10
    assert lib.aware_version() == 350
    with open(os.path.join(ROOT, "include", "aware_hip.h")) as f:
        assert ("int aware_speed_views(const float* in, const int* in_off, const int* in_len, int B, const int* m, int n_views, "
                "float* out,") in f.read()
    for name in ("kernels.h", "capi.hip"):
        with open(os.path.join(ROOT, "aware_amd", "csrc", name)) as f:
            assert "_speed_views(const float* in, const int* in_off, const int* in_len, int B, const int* m, int n_views" in f.read()
    # the interpolation is one header for both kernels
    for name in ("loop_speed_kernels.hip", "speed_search_kernels.hip"):
        with open(os.path.join(ROOT, "aware_amd", "csrc", name)) as f:
            src = f.read()
        assert '#include "speed_interp.hpp"' in src and "speed_weights(float f)" not in src
    assert lib.aware_speed_views(None, None, None, 1, None, 49, None, None, 16000, None) == -1
    p, q = C.c_void_p(256), C.c_void_p(512)                 # never dereferenced: every call below is refused
    for i in range(6):                                      # each pointer in turn
        a = [p, p, p, p, q, p]
        a[i] = None
        assert lib.aware_speed_views(a[0], a[1], a[2], 1, a[3], 49, a[4], a[5], 16000, None) == -1, i
    for B, nv, max_len in ((0, 49, 16000), (-1, 49, 16000), (65536, 49, 16000), (1, 0, 16000), (1, 64, 16000), (1, -3, 16000),
                           (1, 49, 0), (1, 49, -5), (1, 49, (1 << 30) + 1)):
        assert lib.aware_speed_views(p, p, p, B, p, nv, q, p, max_len, None) == -1, (B, nv, max_len)
    assert lib.aware_speed_views(p, p, p, 1, p, 49, p, p, 16000, None) == -1               # in == out


# ---- 5. the value claim, on the CPU ---------------------------------------------------------------------------------------------
def best_views(plain, z, ms, sync_n=0):
    """z [4, n] -> speed_select over the views of the oracle's detector: (values, flat index, confidence, the plain read)."""
    offs = S.sync_offsets(sync_n)
    zt = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32))
    rows = []
    for m in ms:
        view = LA.speed_change(zt, m, LA.speed_length(z.shape[1], m)).numpy()
        rows += [plain.detect_raw(np.ascontiguousarray(view[:, e:])).numpy() for e in offs]
    v = np.stack(rows, axis=1)                                                             # [4, n_speed * n_sync, 20]
    out, idx, conf = S.speed_select(v.reshape(-1, v.shape[-1]), len(ms), sync_n, 0.0)
    return out, idx, conf, v[:, 0]


def test_the_search_recovers_clips_played_at_another_speed():
    """Four 1 s clips embedded plainly (400 steps), then resampled with scipy.signal.resample_poly (another interpolator than
    the views') at seven ratios between x0.90 and x1.10: the plain read-out loses at least a quarter of the bits on average,
    the best of 49 views loses none, the chosen offset lies within one grid step of 65536 (up / down - 1), and its confidence
    is at least three times what unmarked audio reaches over the same views.  With the first 256 samples gone as well, the
    search times 8 sync offsets reads every bit.  Measured: see DESIGN.md section 27."""
    from scipy.signal import resample_poly
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    pairs = [make_clip(s, 16000) for s in range(4)]
    audio = np.stack([p[0] for p in pairs])
    bits = np.stack([p[1] for p in pairs])
    wm = np.stack([O.bits_to_bipolar(b) for b in bits]).astype(np.float32)
    plain = O.Embedder()
    y = plain.embed(audio, wm)[0].numpy()
    ms = S.speed_offsets(GRID)
    delta = ms[2]
    assert delta == 328

    out, idx, conf, _ = best_views(plain, y, ms)
    print(f"no attack: best view m = {[ms[j] for j in idx]}, confidence {[round(float(c), 3) for c in conf]}")
    assert float((O.decode_bits(out) != bits).mean()) == 0.0 and idx.tolist() == [0] * 4   # clean: the plain read, every bit

    _, _, unmarked, _ = best_views(plain, audio[:, :y.shape[1]], ms)
    floor = float(unmarked.max())
    print(f"unmarked hosts: largest confidence over the 49 views {[round(float(c), 4) for c in unmarked]}")

    plain_ber = []
    for up, down in RATIOS:
        z = resample_poly(y, up, down, axis=1).astype(np.float32)
        out, idx, conf, first = best_views(plain, z, ms)
        b0 = 100.0 * float((O.decode_bits(first) != bits).mean())
        b1 = 100.0 * float((O.decode_bits(out) != bits).mean())
        ideal = 65536.0 * (up / down - 1.0)
        chosen = [ms[j] for j in idx]
        print(f"x{down / up:.4f} ({up}/{down}): plain {b0:.2f} % / best of 49 views {b1:.2f} %; m {chosen} (ideal {ideal:.0f}), "
              f"confidence {[round(float(c), 3) for c in conf]}")
        plain_ber.append(b0)
        assert b1 == 0.0, (up, down)
        assert max(abs(m - ideal) for m in chosen) <= delta, (up, down, chosen)
        assert float(conf.min()) >= 3.0 * floor, (up, down, conf, floor)
    assert float(np.mean(plain_ber)) >= 25.0, plain_ber

    z = resample_poly(y[:, 256:], 20, 21, axis=1).astype(np.float32)                       # trimmed, then x1.05
    out, idx, conf, _ = best_views(plain, z, ms, 8)
    print(f"256 samples trimmed, then x1.05: 49 x 8 views, m {[ms[j // 8] for j in idx]}, offsets {[S.sync_offsets(8)[j % 8] for j in idx]}, "
          f"confidence {[round(float(c), 3) for c in conf]}")
    assert float((O.decode_bits(out) != bits).mean()) == 0.0
