"""Speed search in detection (EXTENSION) on the device: the views kernel of csrc/speed_search_kernels.hip (aware_speed_views)
against the existing speed change, bit for bit, and against the float64 restatement; and the search end to end: clips embedded
plainly, resampled by the polyphase attack, read again through AWAREDetector.detect_batch(speed_search=12.0), alone and together
with the offset search.

Run on the MI355X box:  python -m pytest tests/test_gpu_speed_search.py -m gpu -q -s"""
import numpy as np
import pytest
import torch

from conftest import make_clip
from test_gpu_loop_speed import CAP, SPEED_BOUND

pytestmark = pytest.mark.gpu

MS = [0, -1, 1, 328, -7872, 7872, -13107, 13107]
RATIOS = [(20, 21), (20, 19), (10, 11), (10, 9), (400, 431)]       # resample_poly(up, down): played at down / up of the speed
SENTINEL = -777.25


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


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", [[5, 1025, 4099], [1], [2], [3], [255], [1024]], ids=lambda v: "-".join(map(str, v)))
def test_speed_views_match_the_speed_change(rt, LA, lengths):
    """Every view equals aware_speed_change at the same offset and length bit for bit, lies within the bound that
    test_gpu_loop_speed.py allows that kernel against the float64 restatement, and m = 0 copies the clip; nothing is written
    outside the rows.  The clips start 3 floats into their buffer (clip 1 at float 8, clip 2 at float 1033): no input row is
    aligned to 16 bytes.  4099 samples are six workgroups at m = -13107 (5123 outputs) and a partial last group of four at most offsets."""
    rng = np.random.default_rng(sum(lengths))
    xs = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    buf = torch.zeros(3 + sum(lengths), dtype=torch.float32, device="cuda")
    buf[3:] = torch.from_numpy(np.concatenate(xs))
    x = rt.Ragged(buf[3:], lengths)
    assert x.data.data_ptr() % 16 == 12
    want_len = [LA.speed_length(n, m) for n in lengths for m in MS]
    total = sum((n + 3) // 4 * 4 for n in want_len)
    out = torch.full((total + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    flat, vlen, voff = rt.speed_views(x, MS, out=out)
    torch.cuda.synchronize()
    assert flat is out and vlen == want_len and len(voff) == len(lengths) * len(MS)
    assert all(o % 4 == 0 for o in voff) and voff[0] == 0 and all(b >= a + n for a, b, n in zip(voff, voff[1:], vlen))
    got = out.cpu().numpy()
    written = np.zeros(len(got), dtype=bool)
    for o, n in zip(voff, vlen):
        written[o:o + n] = True
    assert written.sum() == sum(vlen) and np.all(got[~written] == SENTINEL)                # the padding and the tail are untouched
    worst = 0.0
    for j, m in enumerate(MS):
        ref = rt.speed_change(x, m, out_lengths=[LA.speed_length(n, m) for n in lengths]).to_list()
        for b, (xi, n) in enumerate(zip(xs, lengths)):
            o, no = voff[b * len(MS) + j], vlen[b * len(MS) + j]
            view = got[o:o + no]
            np.testing.assert_array_equal(view.view(np.uint32), ref[b].view(np.uint32), err_msg=f"clip {b}, m = {m}")
            r64 = LA.speed_change(torch.from_numpy(xi).double(), m, no).numpy()
            err = np.abs(view - r64).max() / np.abs(r64).max()
            worst = max(worst, err)
            assert err < SPEED_BOUND <= CAP, (b, m, err)
            if m == 0:
                np.testing.assert_array_equal(view.view(np.uint32), xi.view(np.uint32))
    print(f"speed_views, lengths {lengths}: largest error / peak against the float64 restatement {worst:.2e}")
    # a fresh buffer of the library's own gives the same views
    flat2, vlen2, voff2 = rt.speed_views(x, MS)
    assert vlen2 == vlen and voff2 == voff
    for o, n in zip(voff, vlen):
        assert torch.equal(flat2[o:o + n], out[o:o + n])


def test_speed_views_refuses_bad_arguments(rt):
    x = rt.Ragged.from_list([np.zeros(100, dtype=np.float32)])
    for ms in ([0, -13521], [17035], [], list(range(64))):
        with pytest.raises(ValueError):
            rt.speed_views(x, ms)
    with pytest.raises(ValueError):
        rt.speed_views(x, [0, 328], out=torch.zeros(100, dtype=torch.float32, device="cuda"))          # too small


# ---- 2. the search end to end -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def embedded(rt):
    """Two 1 s clips embedded plainly on the device, 400 steps."""
    from oracle import aware_oracle as O
    from aware_amd.utils.models import load
    emb, det = load()
    pairs = [make_clip(s, 16000) for s in range(2)]
    clips, bits = [p[0] for p in pairs], np.stack([p[1] for p in pairs])
    wm = np.stack([O.bits_to_bipolar(b) for b in bits]).astype(np.float32)
    ys = [o.cpu().numpy() for o in emb.embed_batch(clips, 16000, wm)]
    return det, ys, bits, O


def resampled(rt, clips, up, down):
    from aware_amd import attacks
    return attacks.resample_poly_batch(rt.Ragged.from_list(clips), up, down).to_list()


def ber(O, vals, bits):
    return 100.0 * float((O.decode_bits(vals.cpu().numpy()) != bits).mean())


def test_speed_search_recovers_resampled_clips(embedded, rt, S):
    """Clips resampled by the polyphase attack at five ratios: the plain read loses at least a quarter of the bits on
    average, the best of 49 views reads every bit at an offset within one grid step of 65536 (up / down - 1)."""
    det, ys, bits, O = embedded
    delta = S.speed_offsets(12.0)[2]
    plain_ber = []
    for up, down in RATIOS:
        z = resampled(rt, ys, up, down)
        plain = det.detect_batch(z, 16000)
        vals, offsets, m, conf = det.detect_batch(z, 16000, speed_search=12.0, return_speed=True)
        torch.cuda.synchronize()
        ideal = 65536.0 * (up / down - 1.0)
        print(f"x{down / up:.4f} ({up}/{down}): plain {ber(O, plain, bits):.2f} % / best of 49 views {ber(O, vals, bits):.2f} %; "
              f"m {m.cpu().tolist()} (ideal {ideal:.0f}), confidence {[round(float(c), 3) for c in conf.cpu()]} against "
              f"{[round(float(c), 3) for c in plain.abs().mean(dim=1).cpu()]} plain")
        plain_ber.append(ber(O, plain, bits))
        assert m.dtype == torch.int32 and offsets.dtype == torch.int32 and conf.dtype == torch.float32 and vals.shape == plain.shape
        np.testing.assert_array_equal(O.decode_bits(vals.cpu().numpy()), bits)
        assert all(v in S.speed_offsets(12.0) and abs(v - ideal) <= delta for v in m.cpu().tolist()), (up, down, m)
        assert offsets.cpu().tolist() == [0, 0]
    assert float(np.mean(plain_ber)) >= 25.0, plain_ber
    # the other forms of the call: the values alone, the 3-tuple of return_sync, detect() on one clip, the dict
    assert torch.equal(det.detect_batch(z, 16000, speed_search=12.0), vals)
    three = det.detect_batch(z, 16000, speed_search={"max_percent": 12.0, "step_percent": 0.5}, return_sync=True)
    assert len(three) == 3 and torch.equal(three[0], vals) and torch.equal(three[1], offsets) and torch.equal(three[2], conf)
    np.testing.assert_array_equal(O.decode_bits(det.detect(z[1], 16000, speed_search=12.0)[None]), bits[1:])


def test_speed_search_off_is_the_plain_call(embedded, rt):
    det, ys, bits, O = embedded
    assert det.speed_search is None and det.sync_search == 0
    z = resampled(rt, ys, 20, 21)
    plain = det.detect_batch(z, 16000)
    for off in (None, 0, {}):
        assert torch.equal(det.detect_batch(z, 16000, speed_search=off), plain)
    vals, offsets, conf = det.detect_batch(z, 16000, sync_search=0, return_sync=True, speed_search=0)
    assert torch.equal(vals, plain) and offsets.cpu().tolist() == [0, 0] and torch.equal(conf, plain.abs().mean(dim=1))
    sync8 = det.detect_batch(z, 16000, sync_search=8, return_sync=True)
    again = det.detect_batch(z, 16000, sync_search=8, return_sync=True, speed_search={})
    assert len(sync8) == len(again) == 3 and all(torch.equal(a, b) for a, b in zip(sync8, again))
    four = det.detect_batch(z, 16000, sync_search=8, return_speed=True)                    # the search off: m = 0
    assert len(four) == 4 and four[2].dtype == torch.int32 and four[2].cpu().tolist() == [0, 0]
    assert torch.equal(four[0], sync8[0]) and torch.equal(four[1], sync8[1]) and torch.equal(four[3], sync8[2])
    # untouched clips with the search on: the plain read wins and every bit is there
    vals, offsets, m, conf = det.detect_batch(ys, 16000, speed_search=12.0, return_speed=True)
    assert m.cpu().tolist() == [0, 0] and offsets.cpu().tolist() == [0, 0]
    np.testing.assert_array_equal(O.decode_bits(vals.cpu().numpy()), bits)
    assert float((vals - det.detect_batch(ys, 16000)).abs().max()) < 1e-3                  # the same view, read in a larger batch


def test_speed_search_with_the_offset_search(embedded, rt, S):
    """The first 256 samples dropped, then x1.05: 49 speeds times 8 offsets read every bit; the speed search alone reads
    something else."""
    det, ys, bits, O = embedded
    z = resampled(rt, [y[256:] for y in ys], 20, 21)
    alone = det.detect_batch(z, 16000, speed_search=12.0)
    vals, offsets, m, conf = det.detect_batch(z, 16000, sync_search=8, speed_search=12.0, return_speed=True)
    torch.cuda.synchronize()
    print(f"256 samples trimmed, then x1.05: speed search alone {ber(O, alone, bits):.2f} %, with 8 offsets {ber(O, vals, bits):.2f} %; "
          f"m {m.cpu().tolist()}, offsets {offsets.cpu().tolist()}, confidence {[round(float(c), 3) for c in conf.cpu()]}")
    np.testing.assert_array_equal(O.decode_bits(vals.cpu().numpy()), bits)
    assert not torch.equal(alone, vals)
    assert all(e in S.sync_offsets(8) for e in offsets.cpu().tolist()) and offsets.dtype == torch.int32
    assert all(abs(v - 65536.0 * (20 / 21 - 1.0)) <= 328 for v in m.cpu().tolist())
    three = det.detect_batch(z, 16000, sync_search=8, speed_search=12.0, return_sync=True)
    assert len(three) == 3 and torch.equal(three[0], vals) and torch.equal(three[1], offsets) and torch.equal(three[2], conf)


def test_speed_search_chunks_and_refuses_short_clips(embedded, rt, S, monkeypatch):
    det, ys, bits, O = embedded
    z = resampled(rt, [ys[0][256:], ys[1][300:], ys[0][256:9000]], 20, 21)                 # ragged
    whole = det.detect_batch(z, 16000, sync_search=8, speed_search=12.0, return_speed=True)
    monkeypatch.setattr(S, "SYNC_MAX_ROWS", 49 * 8)                                        # one clip per aware_detect call
    parts = det.detect_batch(z, 16000, sync_search=8, speed_search=12.0, return_speed=True)
    # a batch of another size may take another conv pipe, so the values are compared as read-outs: the same views, values
    # that differ by far less than the 0.2 or so that decides a bit
    assert torch.equal(whole[1], parts[1]) and torch.equal(whole[2], parts[2])
    assert float((whole[0] - parts[0]).abs().max()) < 1e-3 and float((whole[3] - parts[3]).abs().max()) < 1e-3
    np.testing.assert_array_equal(O.decode_bits(parts[0][:2].cpu().numpy()), bits)
    monkeypatch.setattr(S, "SYNC_MAX_ROWS", 49 * 8 - 1)                                    # one clip's rows alone are too many
    with pytest.raises(ValueError):
        det.detect_batch(z, 16000, sync_search=8, speed_search=12.0)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="clip 1"):
        det.detect_batch([z[0], np.zeros(574, dtype=np.float32)], 16000, speed_search=12.0)
    with pytest.raises(ValueError, match="clip 1"):
        det.detect_batch([z[0], np.zeros(900, dtype=np.float32)], 16000, sync_search=8, speed_search=12.0)
    with pytest.raises(ValueError):
        det.detect_batch(z, 16000, speed_search=16.0)


def test_the_service_and_the_card_key(embedded, rt, tmp_path):
    import os
    import yaml
    from conftest import ROOT
    from aware_amd.service import detect_watermark
    from aware_amd.service.detect import detect_watermark_batch
    from aware_amd.utils.models import load
    det, ys, bits, O = embedded
    z = resampled(rt, ys, 10, 11)
    np.testing.assert_array_equal(np.asarray(detect_watermark(z[0], 16000, det, speed_search=12.0)).reshape(-1)[:20], bits[0])
    got = detect_watermark_batch(z, 16000, det, speed_search=12.0)
    np.testing.assert_array_equal(np.stack([np.asarray(g).reshape(-1)[:20] for g in got]), bits)
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        card = yaml.safe_load(f)
    card["speed_search"] = {"max_percent": 12.0, "step_percent": 0.5}
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    _, searching = load(str(p))
    assert searching.speed_search == {"max_percent": 12.0, "step_percent": 0.5}
    np.testing.assert_array_equal(np.asarray(detect_watermark(z[1], 16000, searching)).reshape(-1)[:20], bits[1])
    stereo = np.column_stack([z[0][:14000], z[0][:14000]])
    np.testing.assert_array_equal(np.asarray(detect_watermark(stereo, 16000, searching)).reshape(-1)[:20], bits[0])
