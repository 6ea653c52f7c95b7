"""Offset search in detection (EXTENSION): the restatement aware_amd/detection/sync.py::sync_select against brute force, the
candidate views, the validation of sync_search on the detector, the card and the service, the C ABI's symbol, and the value
claim on the CPU -- a clip whose start was trimmed reads its bits again once the detector looks at 8 offsets.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, make_clip
from oracle import aware_oracle as O
from aware_amd.detection import sync as S


def brute(values, n, centre):
    """Row by row in Python: the largest mean |v - centre| in float32, the first on a tie."""
    B = len(values) // n
    out, idx, conf = [], [], []
    for b in range(B):
        best, arg = None, 0
        for j in range(n):
            c = np.float32(np.mean(np.abs(values[b * n + j] - np.float32(centre)), dtype=np.float32))
            if best is None or c > best:
                best, arg = c, j
        out.append(values[b * n + arg])
        idx.append(arg)
        conf.append(best)
    return np.stack(out), np.array(idx, dtype=np.int32), np.array(conf, dtype=np.float32)


def select_inputs(B, n, L, seed, centre=0.0):
    """Random rows around `centre` with one clear winner per clip (scaled by 2: its confidence is at least a tenth above every other)."""
    rng = np.random.default_rng(seed)
    v = (centre + 0.2 * rng.uniform(0.5, 0.9, size=(B * n, L)) * rng.choice([-1.0, 1.0], size=(B * n, L))).astype(np.float32)
    win = rng.integers(0, n, size=B)
    for b in range(B):
        v[b * n + win[b]] = (centre + 2.0 * (v[b * n + win[b]] - centre)).astype(np.float32)
    return v, win.astype(np.int32)


def tie_inputs(B, n, L, seed):
    """The winner's row duplicated at a later (and, where there is room, an earlier) place: the smallest j is kept."""
    v, win = select_inputs(B, n, L, seed)
    first = win.copy()
    for b in range(B):
        j = (int(win[b]) + 1 + b) % n
        v[b * n + j] = v[b * n + win[b]]
        first[b] = min(int(win[b]), j)
    return v, first


# ---- 1. sync_select ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 8, 64])
@pytest.mark.parametrize("L", [1, 20, 512])
@pytest.mark.parametrize("centre", [0.0, 0.5])
def test_sync_select_is_brute_force(n, L, centre):
    v, win = select_inputs(3, n, L, 100 * n + L, centre)
    out, idx, conf = S.sync_select(v, n, centre)
    assert out.dtype == np.float32 and out.shape == (3, L) and idx.dtype == np.int32 and conf.dtype == np.float32
    bo, bi, bc = brute(v, n, centre)
    np.testing.assert_array_equal(idx, win)
    np.testing.assert_array_equal(idx, bi)
    np.testing.assert_array_equal(out.view(np.uint32), bo.view(np.uint32))
    np.testing.assert_allclose(conf, bc, rtol=1e-6)
    # torch in, torch out
    to, ti, tc = S.sync_select(torch.from_numpy(v), n, centre)
    assert torch.is_tensor(to) and ti.dtype == torch.int32 and tc.dtype == torch.float32
    np.testing.assert_array_equal(to.numpy(), out)
    np.testing.assert_array_equal(ti.numpy(), idx)


@pytest.mark.parametrize("n", [2, 8, 64])
def test_ties_go_to_the_smallest_index(n):
    v, first = tie_inputs(3, n, 20, n)
    out, idx, conf = S.sync_select(v, n, 0.0)
    np.testing.assert_array_equal(idx, first)
    np.testing.assert_array_equal(idx, brute(v, n, 0.0)[1])
    same = np.tile(v[:1], (n, 1))                                                          # every row equal: j = 0
    assert int(S.sync_select(same, n)[1][0]) == 0


def test_sync_select_refuses_bad_shapes():
    for v, n in ((np.zeros((7, 4), np.float32), 2), (np.zeros((0, 4), np.float32), 2), (np.zeros(8, np.float32), 2),
                 (np.zeros((8, 4), np.float32), 0)):
        with pytest.raises(ValueError):
            S.sync_select(v, n)


# ---- 2. the views and the validation ------------------------------------------------------------------------------------------------
def test_views_and_offsets():
    assert S.SYNC_PERIOD == 512 and S.SYNC_CHOICES == (2, 4, 8, 16, 32, 64)
    assert S.sync_offsets(8) == [0, 64, 128, 192, 256, 320, 384, 448]
    assert S.sync_offsets(2) == [0, 256] and S.sync_offsets(64)[-1] == 504 and S.sync_offsets(0) == [0]
    vlen, voff = S.sync_views([16000, 1000], 4)
    assert vlen == [16000, 15872, 15744, 15616, 1000, 872, 744, 616] and voff == [0, 128, 256, 384] * 2
    with pytest.raises(ValueError, match="clip 1"):
        S.sync_views([16000, 900], 8)                                                      # 900 - 448 = 452 <= 512
    S.sync_views([961], 8)                                                                 # 513 samples are left
    with pytest.raises(ValueError):
        S.sync_views([960], 8)


@pytest.mark.parametrize("n", [3, 5, 6, 12, 128, -1, 2.0, "8", True])
def test_bad_sync_search_is_refused(n):
    with pytest.raises(ValueError):
        S.check_sync_search(n)
    from aware_amd.detection import AWAREDetector
    with pytest.raises(ValueError):
        AWAREDetector(model=None, sync_search=n)


def test_sync_search_defaults_off():
    assert [S.check_sync_search(n) for n in (None, 0, 1, 2, 4, 8, 16, 32, 64, np.int64(8))] == [0, 0, 0, 2, 4, 8, 16, 32, 64, 8]
    from aware_amd.detection import AWAREDetector
    det = AWAREDetector(model=None)
    assert det.sync_search == 0
    assert AWAREDetector(model=None, sync_search=8).sync_search == 8 and AWAREDetector(model=None, sync_search=1).sync_search == 0
    import inspect
    from aware_amd.service import detect as SD
    assert inspect.signature(det.detect_batch).parameters["sync_search"].default is None
    assert inspect.signature(det.detect_batch).parameters["return_sync"].default is False
    assert inspect.signature(det.detect).parameters["sync_search"].default is None
    assert inspect.signature(SD.detect_watermark).parameters["sync_search"].default is None
    assert inspect.signature(SD.detect_watermark_batch).parameters["sync_search"].default is None


def test_the_service_keeps_the_plain_call_when_the_search_is_off():
    """A detector that knows nothing of the search is called exactly as before; a detector with one is asked for it."""
    from aware_amd.service.detect import detect_watermark, detect_watermark_batch

    class Plain:
        pattern_mode, threshold = "bits2bipolar", 0.0

        def detect(self, audio, sr):
            return np.array([0.5, -0.5], dtype=np.float32)

        def detect_batch(self, clips, sr):
            return torch.tensor([[0.5, -0.5]] * len(clips))

    class Searching(Plain):
        sync_search = 8
        calls = []

        def detect_batch(self, clips, sr, sync_search=None, return_sync=False):
            self.calls.append((sync_search, return_sync))
            v = torch.tensor([[0.5, -0.5]] * len(clips))
            return (v, torch.zeros(len(clips), dtype=torch.int32), torch.ones(len(clips))) if return_sync else v

    a = np.zeros(2000, dtype=np.float32)
    want = list(detect_watermark(a, 16000, Plain()))
    assert list(detect_watermark(np.stack([a, a], axis=1), 16000, Plain())) == want
    assert [list(b) for b in detect_watermark_batch([a, a], 16000, Plain())] == [want, want]
    s = Searching()
    assert list(detect_watermark(a, 16000, s)) == want and s.calls[-1] == (None, True)
    assert list(detect_watermark(a, 16000, s, sync_search=4)) == want and s.calls[-1] == (4, True)
    assert [list(b) for b in detect_watermark_batch([a], 16000, s, sync_search=0)] == [want] and s.calls[-1] == (0, True)


def test_card_key_reaches_the_detector(tmp_path):
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        text = f.read()
    assert "# sync_search: 8" in text
    card = yaml.safe_load(text)
    assert "sync_search" not in card
    assert load()[1].sync_search == 0                                                      # the committed card keeps its behaviour
    card["sync_search"] = 8
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    assert load(str(p))[1].sync_search == 8
    card["sync_search"] = 3
    p.write_text(yaml.safe_dump(card))
    assert load(str(p)) is None


def test_abi_symbol_and_bad_arguments():
    from aware_amd import _lib
    lib = _lib.load_library()
    assert "aware_sync_select" in _lib.SIGNATURES and hasattr(lib, "aware_sync_select")
    assert "sync_kernels.hip" in _lib.SOURCES and len(_lib.SIGNATURES["aware_sync_select"][1]) == 9
    assert lib.aware_version() == 350
    with open(os.path.join(ROOT, "include", "aware_hip.h")) as f:
        assert "int aware_sync_select(const float* values, int B, int n, int L, float centre" in f.read()
    assert lib.aware_sync_select(None, 1, 8, 20, 0.0, None, None, None, None) == -1
    p, q = C.c_void_p(256), C.c_void_p(512)                 # never dereferenced: every call below is refused
    for i in range(4):                                      # each pointer in turn
        a = [p, q, q, q]
        a[i] = None
        assert lib.aware_sync_select(a[0], 1, 8, 20, 0.0, a[1], a[2], a[3], None) == -1, i
    for B, n, L, centre in ((0, 8, 20, 0.0), (65536, 8, 20, 0.0), (1, 0, 20, 0.0), (1, 65, 20, 0.0), (1, 8, 0, 0.0),
                            (1, 8, 65537, 0.0), (1, 8, 20, float("nan")), (1, 8, 20, float("inf"))):
        assert lib.aware_sync_select(p, B, n, L, centre, q, q, q, None) == -1, (B, n, L, centre)
    assert lib.aware_sync_select(p, 1, 8, 20, 0.0, p, q, q, None) == -1                    # out_values == values


# ---- 3. the value claim, on the CPU ---------------------------------------------------------------------------------------------
def test_the_search_recovers_trimmed_clips():
    """Four 1 s clips embedded plainly (400 steps), the first d samples dropped, d in {224, 256, 288}: the plain read-out loses
    at least 10 % of the bits on average, the best of 8 views of the oracle's detector loses none, and the chosen offset lies
    within 64 samples, circularly, of (-d) mod 512.  Measured: see DESIGN.md section 21."""
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    pairs = [make_clip(s, 16000) for s in range(4)]
    audio = np.stack([p[0] for p in pairs])
    bits = np.stack([p[1] for p in pairs])
    wm = np.stack([O.bits_to_bipolar(b) for b in bits]).astype(np.float32)
    plain = O.Embedder()
    y = plain.embed(audio, wm)[0].numpy()
    offs = S.sync_offsets(8)
    plain_ber, search_ber = [], []
    for d in (224, 256, 288):
        z = y[:, d:]
        views = [plain.detect_raw(np.ascontiguousarray(z[:, e:], dtype=np.float32)).numpy() for e in offs]       # 8 x [4, 20]
        v = np.stack(views, axis=1).reshape(4 * 8, -1)                                     # clip-major
        out, idx, conf = S.sync_select(v, 8, 0.0)
        b0 = 100.0 * float((O.decode_bits(views[0]) != bits).mean())
        b1 = 100.0 * float((O.decode_bits(out) != bits).mean())
        chosen = [offs[j] for j in idx]
        want = (-d) % 512
        dist = [min((c - want) % 512, (want - c) % 512) for c in chosen]
        print(f"first {d} samples dropped: plain {b0:.2f} % / best of 8 views {b1:.2f} %; offsets {chosen} (aligned at {want}), "
              f"confidence {[round(float(c), 3) for c in conf]} against {[round(float(np.abs(views[0][b]).mean()), 3) for b in range(4)]} at e = 0")
        plain_ber.append(b0)
        search_ber.append(b1)
        assert max(dist) <= 64, (d, chosen)
    assert float(np.mean(plain_ber)) >= 10.0
    assert search_ber == [0.0, 0.0, 0.0]
