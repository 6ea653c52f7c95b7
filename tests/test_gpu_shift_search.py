"""Shift search in detection (EXTENSION) on the device: the views kernel of csrc/shift_search_kernels.hip (aware_shift_views)
against the stand-alone frequency shift, bit for bit, and against the float64 restatement; and the search end to end: clips
embedded plainly, moved by a constant number of Hz on the host (FFT analytic signal), read again through
AWAREDetector.detect_batch_shift(shift_search=150), alone and together with the offset search.

Run on the MI355X box:  python -m pytest tests/test_gpu_shift_search.py -m gpu -q -s"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import make_clip
from test_gpu_loop_shift import bound_of            # 2^-16 (1 + sum|h|) max|x|: the stand-alone operator's output bound

pytestmark = pytest.mark.gpu

DRAW = [0, 1, -1, 655, -655, 3277, -3277, 65536, -65536]   # the shifts a view is drawn from; the ends are the operator's range
SENTINEL = -777.25
SHIFTS_HZ = [50.0, -77.0, 123.4]
LENGTHS = [[5, 1025, 4099], [1], [2], [255], [4095], [4096], [4097], [8191, 3]]


@pytest.fixture(scope="module")
def rt():
    from aware_amd import runtime
    from aware_amd._lib import require_gpu
    require_gpu()
    return runtime


@pytest.fixture(scope="module")
def S():
    from aware_amd.detection import sync
    return sync


@pytest.fixture(scope="module")
def LA():
    from aware_amd.embedding import loop_attacks
    return loop_attacks


def shifts_of(n_views):
    """n_views shifts from DRAW, 0 first; with 63 views every value several times, in an order of its own."""
    if n_views <= len(DRAW):
        return {1: [0], 3: [0, -655, 65536]}.get(n_views, DRAW[:n_views])
    rng = np.random.default_rng(n_views)
    return [0] + [DRAW[i] for i in rng.integers(0, len(DRAW), size=n_views - 1)]


def misaligned(rt, xs):
    """The clips back to back from 3 floats into their buffer: data_ptr() % 16 == 12, no input row aligned to 16 bytes by design."""
    buf = torch.zeros(3 + sum(len(x) for x in xs), dtype=torch.float32, device="cuda")
    buf[3:] = torch.from_numpy(np.concatenate(xs))
    x = rt.Ragged(buf[3:], [len(x) for x in xs])
    assert x.data.data_ptr() % 16 == 12
    return x


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_views", [1, 3, 63])
@pytest.mark.parametrize("lengths", LENGTHS, ids=lambda v: "-".join(map(str, v)))
def test_shift_views_match_the_frequency_shift(rt, lengths, n_views):
    """Every view equals aware_frequency_shift at the same shift and the start phase 0 bit for bit, d = 0 gives the clip's own
    bits, and nothing is written outside the rows.  4095, 4096 and 4097 samples end a sample before, at and behind the edge of
    a workgroup's tile of 4096; 8191 are two tiles, the first one's halo reaching into the second; 1 to 255 are shorter than
    the taps."""
    rng = np.random.default_rng(sum(lengths) + n_views)
    xs = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    for x in xs:                                            # non-zero up to both ends: a halo that reads a neighbour shows
        x[0], x[-1] = 1.5, -1.5
    x = misaligned(rt, xs)
    ds = shifts_of(n_views)
    assert len(ds) == n_views and ds[0] == 0
    want_len = [n for n in lengths for _ in ds]
    total = sum((n + 3) // 4 * 4 for n in want_len)
    out = torch.full((total + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    flat, vlen, voff = rt.shift_views(x, ds, out=out)
    torch.cuda.synchronize()
    assert flat is out and vlen == want_len and len(voff) == len(lengths) * n_views
    assert all(o % 4 == 0 for o in voff) and voff[0] == 0 and all(b >= a + n for a, b, n in zip(voff, voff[1:], vlen))
    got = out.cpu().numpy()
    written = np.zeros(len(got), dtype=bool)
    for o, n in zip(voff, vlen):
        written[o:o + n] = True
    assert written.sum() == sum(vlen) and np.all(got[~written] == SENTINEL)                # the padding and the tail are untouched
    refs = {d: rt.frequency_shift(x, d, 0).to_list() for d in sorted(set(ds))}
    for j, d in enumerate(ds):
        for b, xi in enumerate(xs):
            o, n = voff[b * n_views + j], vlen[b * n_views + j]
            view = got[o:o + n]
            np.testing.assert_array_equal(view.view(np.uint32), refs[d][b].view(np.uint32), err_msg=f"clip {b}, view {j}, d = {d}")
            if d == 0:
                np.testing.assert_array_equal(view.view(np.uint32), xi.view(np.uint32))
    # a fresh buffer of the library's own gives the same views
    flat2, vlen2, voff2 = rt.shift_views(x, ds)
    assert vlen2 == vlen and voff2 == voff
    for o, n in zip(voff, vlen):
        assert torch.equal(flat2[o:o + n], out[o:o + n])


def test_shift_views_against_the_float64_restatement(rt, LA):
    """Directly against loop_attacks.frequency_shift in float64, at the stand-alone operator's output bound
    2^-16 (1 + sum|h|) max|x| of test_gpu_loop_shift.py."""
    lengths = [4099, 255, 8193]
    rng = np.random.default_rng(39)
    xs = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    ds = [0, 655, -3277, 65536, -65536, 1, -9825]
    flat, vlen, voff = rt.shift_views(misaligned(rt, xs), ds)
    got = flat.cpu().numpy()
    worst = 0.0
    for b, xi in enumerate(xs):
        bound = bound_of(np.abs(xi).max())
        for j, d in enumerate(ds):
            o = voff[b * len(ds) + j]
            ref = LA.frequency_shift(torch.from_numpy(xi).double(), d, 0).numpy()
            err = float(np.abs(got[o:o + len(xi)].astype(np.float64) - ref).max())
            worst = max(worst, err / bound)
            assert err <= bound, (b, d, err, bound)
    print(f"shift_views against the float64 restatement: largest error / bound {worst:.4f}")


def test_shift_views_refuses_bad_arguments(rt):
    from aware_amd import _lib
    x = rt.Ragged.from_list([np.zeros(100, dtype=np.float32)])
    for ds in ([0, 65537], [-65537], [], list(range(64))):                                 # refused before the launch
        with pytest.raises(ValueError):
            rt.shift_views(x, ds)
    with pytest.raises(ValueError):
        rt.shift_views(x, [0, 655], out=torch.zeros(100, dtype=torch.float32, device="cuda"))          # too small
    lib = _lib.load_library()
    d = torch.zeros(3, dtype=torch.int32, device="cuda")
    oo = torch.tensor([0, 100, 200], dtype=torch.int32, device="cuda")
    out = torch.full((300,), SENTINEL, dtype=torch.float32, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    args = [ptr(x.data), ptr(x.d_off), ptr(x.d_len), 1, ptr(d), 3, ptr(out), ptr(oo), 100, None]
    for i in (0, 1, 2, 4, 6, 7):                                                           # each pointer null in turn
        bad = list(args)
        bad[i] = None
        assert lib.aware_shift_views(*bad) == -1, i
    for i, v in ((5, 0), (5, -1), (5, 64), (3, 0), (3, -2), (8, 0)):                       # n_views < 1 or > 63, B < 1, max_len < 1
        bad = list(args)
        bad[i] = v
        assert lib.aware_shift_views(*bad) == -1, (i, v)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                                   # nothing was launched
    # a shift outside the operator's range that reaches the kernel writes no view; its neighbours are written
    d2 = torch.tensor([0, 65537, -655], dtype=torch.int32, device="cuda")
    args[4] = ptr(d2)
    assert lib.aware_shift_views(*args) == 0
    torch.cuda.synchronize()
    assert bool((out[100:200] == SENTINEL).all()) and bool((out[:100] == 0).all()) and bool((out[200:] == 0).all())


# ---- 2. the search end to end -----------------------------------------------------------------------------------------------------
def ssb(y, hz, sr=16000):
    """Re(analytic(y) e^{j 2 pi hz t}) with the FFT analytic signal: a construction independent of the views' FIR."""
    n = len(y)
    spec = np.fft.fft(np.asarray(y, dtype=np.float64))
    gain = np.zeros(n)
    gain[0] = 1.0
    gain[1:(n + 1) // 2] = 2.0
    if n % 2 == 0:
        gain[n // 2] = 1.0
    return np.real(np.fft.ifft(spec * gain) * np.exp(2j * np.pi * hz * np.arange(n) / sr)).astype(np.float32)


@pytest.fixture(scope="module")
def embedded(rt):
    """Four 1 s clips embedded plainly on the device, 400 steps; the received clips at every shift, made once on the host."""
    from oracle import aware_oracle as O
    from aware_amd.utils.models import load
    emb, det = load()
    pairs = [make_clip(s, 16000) for s in range(4)]
    clips, bits = [p[0] for p in pairs], np.stack([p[1] for p in pairs])
    wm = np.stack([O.bits_to_bipolar(b) for b in bits]).astype(np.float32)
    ys = [o.cpu().numpy() for o in emb.embed_batch(clips, 16000, wm)]
    received = {hz: [ssb(y, hz) for y in ys] for hz in SHIFTS_HZ}
    return det, ys, bits, O, received


def ber(O, vals, bits):
    return 100.0 * float((O.decode_bits(vals.cpu().numpy()) != bits).mean())


def test_shift_search_recovers_shifted_clips(embedded, rt, S):
    """Clips moved by +50, -77 and +123.4 Hz: the plain read loses at least a quarter of the bits on average; the best of the
    31 views of shift_search = 150 undoes the shift to within one grid step, reads no more bits wrongly than the same detector
    on that view made by aware_frequency_shift and detected on its own, and agrees with that read to 1e-3 (the same view, read
    in a larger batch)."""
    det, ys, bits, O, received = embedded
    grid = S.shift_offsets(150, 16000)
    plain_ber = []
    for hz in SHIFTS_HZ:
        z = received[hz]
        plain = det.detect_batch(z, 16000)
        vals, offsets, d, conf = det.detect_batch_shift(z, 16000, shift_search=150, return_shift=True)
        torch.cuda.synchronize()
        found = [S.shift_of(v, 16000) for v in d.cpu().tolist()]
        own = det.detect_batch(rt.frequency_shift(rt.Ragged.from_list(z), d.cpu().tolist(), 0).to_list(), 16000)
        print(f"{hz:+.1f} Hz: plain {ber(O, plain, bits):.2f} % / best of 31 views {ber(O, vals, bits):.2f} % / the chosen view alone "
              f"{ber(O, own, bits):.2f} %; found {[round(f, 1) for f in found]} Hz, confidence {[round(float(c), 3) for c in conf.cpu()]} "
              f"against {[round(float(c), 3) for c in plain.abs().mean(dim=1).cpu()]} plain")
        plain_ber.append(ber(O, plain, bits))
        assert d.dtype == torch.int32 and offsets.dtype == torch.int32 and conf.dtype == torch.float32
        assert vals.shape == plain.shape and d.shape == offsets.shape == conf.shape == (4,)
        assert all(v in grid for v in d.cpu().tolist()) and max(abs(f - hz) for f in found) <= 10.0, (hz, found)
        assert offsets.cpu().tolist() == [0] * 4
        assert ber(O, vals, bits) <= ber(O, own, bits), hz
        assert float((vals - own).abs().max()) < 1e-3, hz
        assert float((conf - own.abs().mean(dim=1)).abs().max()) < 1e-3, hz
    print(f"plain mean BER {np.mean(plain_ber):.2f} %")
    assert float(np.mean(plain_ber)) >= 25.0, plain_ber
    # the other forms: the values alone, the dict, the detector's own key through detect_batch, detect() and return_sync
    from aware_amd.detection import AWAREDetector
    assert torch.equal(det.detect_batch_shift(z, 16000, shift_search={"max_hz": 150, "step_hz": 10}), vals)
    own_key = AWAREDetector(model=det.detection_net, shift_search=150, pattern_mode=det.pattern_mode, threshold=det.threshold,
                            embedding_bands=det.embedding_bands)
    assert torch.equal(own_key.detect_batch(z, 16000), vals)
    three = own_key.detect_batch(z, 16000, return_sync=True)
    assert len(three) == 3 and torch.equal(three[0], vals) and torch.equal(three[1], offsets) and torch.equal(three[2], conf)
    four = own_key.detect_batch(z, 16000, return_speed=True)                               # no speed was searched: m = 0
    assert len(four) == 4 and torch.equal(four[0], vals) and four[2].cpu().tolist() == [0] * 4 and torch.equal(four[3], conf)
    assert float(np.abs(own_key.detect(z[1], 16000) - vals[1].cpu().numpy()).max()) < 1e-3
    with pytest.raises(ValueError, match="scan: shift_search"):
        own_key.scan(z, 16000)
    with pytest.raises(ValueError, match="speed_search and shift_search"):
        own_key.detect_batch(z, 16000, speed_search=12.0)


def test_shift_search_off_is_the_plain_call(embedded, rt):
    det, ys, bits, O, received = embedded
    assert det.shift_search is None and det.speed_search is None and det.sync_search == 0
    z = received[50.0]
    plain = det.detect_batch(z, 16000)
    for off in (None, 0, {}, False):
        assert torch.equal(det.detect_batch_shift(z, 16000, shift_search=off), plain)
    vals, offsets, d, conf = det.detect_batch_shift(z, 16000, return_shift=True)           # the search off: d = 0
    assert torch.equal(vals, plain) and offsets.cpu().tolist() == [0] * 4 and d.cpu().tolist() == [0] * 4
    assert d.dtype == torch.int32 and torch.equal(conf, plain.abs().mean(dim=1))
    sync8 = det.detect_batch(z, 16000, sync_search=8, return_sync=True)
    four = det.detect_batch_shift(z, 16000, sync_search=8, shift_search=0, return_shift=True)
    assert torch.equal(four[0], sync8[0]) and torch.equal(four[1], sync8[1]) and torch.equal(four[3], sync8[2])
    # untouched clips with the search on: the plain read wins
    vals, offsets, d, conf = det.detect_batch_shift(ys, 16000, shift_search=150, return_shift=True)
    assert d.cpu().tolist() == [0] * 4 and offsets.cpu().tolist() == [0] * 4
    assert float((vals - det.detect_batch(ys, 16000)).abs().max()) < 1e-3                  # the same view, read in a larger batch


def test_shift_search_with_the_offset_search(embedded, rt, S):
    """Moved by 50 Hz, then the first 224 samples dropped: 31 shifts times 8 offsets find the shift to within 10 Hz and an
    offset within 64 samples of the 288 that complete the period of 512, and read what the same detector reads on that view alone."""
    det, ys, bits, O, received = embedded
    z = [v[224:] for v in received[50.0]]
    vals, offsets, d, conf = det.detect_batch_shift(z, 16000, sync_search=8, shift_search=150, return_shift=True)
    torch.cuda.synchronize()
    found = [S.shift_of(v, 16000) for v in d.cpu().tolist()]
    views = rt.frequency_shift(rt.Ragged.from_list(z), d.cpu().tolist(), 0).to_list()
    own = det.detect_batch([v[e:] for v, e in zip(views, offsets.cpu().tolist())], 16000)
    print(f"+50 Hz, then 224 samples trimmed: 31 x 8 views {ber(O, vals, bits):.2f} %, the chosen view alone {ber(O, own, bits):.2f} %; "
          f"found {[round(f, 1) for f in found]} Hz, offsets {offsets.cpu().tolist()}, confidence {[round(float(c), 3) for c in conf.cpu()]}")
    assert offsets.dtype == torch.int32 and all(e in S.sync_offsets(8) and abs(e - 288) <= 64 for e in offsets.cpu().tolist())
    assert max(abs(f - 50.0) for f in found) <= 10.0, found
    assert ber(O, vals, bits) <= ber(O, own, bits) and float((vals - own).abs().max()) < 1e-3


def test_shift_search_chunks_and_refuses_short_clips(embedded, rt, S, monkeypatch):
    det, ys, bits, O, received = embedded
    z = [received[-77.0][0], received[-77.0][1][300:], received[-77.0][2][:9000]]          # ragged
    whole = det.detect_batch_shift(z, 16000, shift_search=150, return_shift=True)
    monkeypatch.setattr(S, "SYNC_MAX_ROWS", 31)                                            # one clip per aware_detect call
    parts = det.detect_batch_shift(z, 16000, shift_search=150, return_shift=True)
    # a batch of another size may take another conv pipe, so the values are compared as read-outs
    assert torch.equal(whole[1], parts[1]) and torch.equal(whole[2], parts[2])
    assert float((whole[0] - parts[0]).abs().max()) < 1e-3 and float((whole[3] - parts[3]).abs().max()) < 1e-3
    monkeypatch.setattr(S, "SYNC_MAX_ROWS", 30)                                            # one clip's rows alone are too many
    with pytest.raises(ValueError, match="shift_search"):
        det.detect_batch_shift(z, 16000, shift_search=150)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="clip 1"):
        det.detect_batch_shift([z[0], np.zeros(512, dtype=np.float32)], 16000, shift_search=150)
    with pytest.raises(ValueError, match="clip 1"):
        det.detect_batch_shift([z[0], np.zeros(960, dtype=np.float32)], 16000, sync_search=8, shift_search=150)
    with pytest.raises(ValueError):
        det.detect_batch_shift(z, 16000, shift_search=320)                                 # 65 views


def test_the_service_and_the_card_key(embedded, rt, tmp_path):
    import os
    import yaml
    from conftest import ROOT
    from aware_amd.service import detect_watermark
    from aware_amd.service.detect import detect_watermark_batch
    from aware_amd.utils.models import load
    det, ys, bits, O, received = embedded
    z = received[50.0]
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        card = yaml.safe_load(f)
    card["shift_search"] = 100
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    _, searching = load(str(p))
    assert searching.shift_search == {"max_hz": 100.0, "step_hz": 10.0}
    vals = searching.detect_batch(z, 16000).cpu().numpy()
    clear = np.abs(vals) > 1e-2                               # a batch of another size reads values within 1e-3: these bits are decided
    want = O.decode_bits(vals)
    print(f"card key shift_search: 100 on +50 Hz: {100.0 * float((want != bits).mean()):.2f} % of the bits wrong")

    def rows(got):
        return np.stack([np.asarray(g).reshape(-1)[:20] for g in got])

    np.testing.assert_array_equal(rows(detect_watermark_batch(z, 16000, searching)), want)
    np.testing.assert_array_equal(rows([detect_watermark(z[1], 16000, searching)])[0][clear[1]], want[1][clear[1]])
    stereo = np.column_stack([z[0], z[0]])
    np.testing.assert_array_equal(rows([detect_watermark(stereo, 16000, searching)])[0][clear[0]], want[0][clear[0]])
    # the plain detector's service calls are what they were
    plain = O.decode_bits(det.detect_batch(z, 16000).cpu().numpy())
    np.testing.assert_array_equal(rows(detect_watermark_batch(z, 16000, det)), plain)
