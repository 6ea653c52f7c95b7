"""Offset search in detection (EXTENSION) on the device: the selection kernel of csrc/sync_kernels.hip (aware_sync_select)
against the restatement aware_amd/detection/sync.py::sync_select, and the search end to end: clips embedded plainly, their
start trimmed, read again through AWAREDetector.detect_batch(sync_search=8).

Run on the MI355X box:  python -m pytest tests/test_gpu_sync_search.py -m gpu -q -s"""
import numpy as np
import pytest
import torch

from conftest import make_clip
from test_sync_search_host import select_inputs, tie_inputs

pytestmark = pytest.mark.gpu


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


def confidences(v, n, centre):
    B = len(v) // n
    return np.abs(v.astype(np.float64) - centre).mean(axis=1).reshape(B, n)


# ---- 1. the selection kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 8, 64])
@pytest.mark.parametrize("L", [1, 20, 512])
def test_sync_select_matches_the_restatement(rt, S, n, L):
    """B = 3; clear winners (around 0 and around 0.5) and exact ties: the chosen index and the copied row bit for bit, the
    confidence within float32 rounding of the mean.  Wherever two confidences are not exactly tied, the top two differ by more
    than 1 % (checked here in float64), so the order of a float32 sum cannot decide a case."""
    cases = [select_inputs(3, n, L, 100 * n + L, 0.0) + (0.0,), select_inputs(3, n, L, 100 * n + L, 0.5) + (0.5,),
             tie_inputs(3, n, L, n + L) + (0.0,)]
    for v, want, centre in cases:
        c = confidences(v, n, centre)
        for b in range(3):
            top = np.sort(c[b])[::-1]
            others = top[top < top[0]]
            assert len(others) == 0 or others[0] < 0.99 * top[0], (b, top[:3])
        ref_out, ref_idx, ref_conf = S.sync_select(v, n, centre)
        np.testing.assert_array_equal(ref_idx, want)
        out, idx, conf = rt.sync_select(torch.from_numpy(v).cuda(), n, centre)
        torch.cuda.synchronize()
        assert out.shape == (3, L) and idx.dtype == torch.int32 and conf.dtype == torch.float32
        np.testing.assert_array_equal(idx.cpu().numpy(), ref_idx)
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), ref_out.view(np.uint32))
        # L terms of one sign, each rounded once and summed in float32: within L * 2^-24 of the exact mean, relatively
        np.testing.assert_allclose(conf.cpu().numpy(), c[np.arange(3), ref_idx], rtol=(L + 2) * 2.0 ** -24)
    same = np.tile(cases[0][0][:1], (3 * n, 1))                                            # every row equal: j = 0
    assert rt.sync_select(torch.from_numpy(same).cuda(), n)[1].cpu().tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        rt.sync_select(torch.zeros((7, 4), device="cuda"), 2)


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


def test_sync_search_off_is_the_plain_call(embedded):
    det, ys, bits, O = embedded
    assert det.sync_search == 0
    trimmed = [y[256:] for y in ys]
    plain = det.detect_batch(trimmed, 16000)
    for n in (0, 1, None):
        assert torch.equal(det.detect_batch(trimmed, 16000, sync_search=n), plain)
    vals, offsets, conf = det.detect_batch(trimmed, 16000, sync_search=0, return_sync=True)
    assert torch.equal(vals, plain) and offsets.cpu().tolist() == [0, 0] and conf.shape == (2,)
    np.testing.assert_array_equal(O.decode_bits(det.detect_batch(ys, 16000).cpu().numpy()), bits)       # untrimmed: all bits


@pytest.mark.parametrize("d", [224, 256, 300])
def test_sync_search_recovers_trimmed_clips(embedded, S, d):
    """The first d samples dropped: the best of 8 views reads every bit, at an offset within 64 samples, circularly, of
    (-d) mod 512."""
    det, ys, bits, O = embedded
    trimmed = [y[d:] for y in ys]
    plain = det.detect_batch(trimmed, 16000)
    vals, offsets, conf = det.detect_batch(trimmed, 16000, sync_search=8, return_sync=True)
    torch.cuda.synchronize()
    b0 = 100.0 * float((O.decode_bits(plain.cpu().numpy()) != bits).mean())
    b1 = 100.0 * float((O.decode_bits(vals.cpu().numpy()) != bits).mean())
    want = (-d) % 512
    offs = offsets.cpu().tolist()
    print(f"first {d} samples dropped: plain {b0:.2f} % / best of 8 views {b1:.2f} %; offsets {offs} (aligned at {want}), confidence "
          f"{[round(float(c), 3) for c in conf.cpu()]} against {[round(float(c), 3) for c in plain.abs().mean(dim=1).cpu()]} at e = 0")
    assert offsets.dtype == torch.int32 and conf.dtype == torch.float32 and vals.shape == plain.shape
    np.testing.assert_array_equal(O.decode_bits(vals.cpu().numpy()), bits)
    assert all(e in S.sync_offsets(8) and min((e - want) % 512, (want - e) % 512) <= 64 for e in offs), offs
    assert torch.equal(det.detect_batch(trimmed, 16000, sync_search=8), vals)              # without return_sync: the values alone
    np.testing.assert_array_equal(O.decode_bits(det.detect(trimmed[1], 16000, sync_search=8)[None]), bits[1:])


def test_sync_search_chunks_and_refuses_short_clips(embedded, S, monkeypatch):
    det, ys, bits, O = embedded
    trimmed = [ys[0][256:], ys[1][300:], ys[0][256:9000]]                                  # ragged
    whole = det.detect_batch(trimmed, 16000, sync_search=8, return_sync=True)
    monkeypatch.setattr(S, "SYNC_MAX_ROWS", 8)                                             # one clip per aware_detect call
    parts = det.detect_batch(trimmed, 16000, sync_search=8, return_sync=True)
    # a batch of another size may take another conv pipe, so the values are compared as read-outs: the same views, values
    # that differ by far less than the 0.2 or so that decides a bit
    assert torch.equal(whole[1], parts[1])
    assert float((whole[0] - parts[0]).abs().max()) < 1e-3 and float((whole[2] - parts[2]).abs().max()) < 1e-3
    np.testing.assert_array_equal(O.decode_bits(parts[0][:2].cpu().numpy()), bits)
    with pytest.raises(ValueError, match="clip 1"):
        det.detect_batch([trimmed[0], np.zeros(900, dtype=np.float32)], 16000, sync_search=8)
    with pytest.raises(ValueError):
        det.detect_batch(trimmed, 16000, sync_search=3)


def test_the_service_and_the_card_key(embedded, tmp_path):
    import os
    import yaml
    from conftest import ROOT
    from aware_amd.service import detect_watermark
    from aware_amd.service.detect import detect_watermark_batch
    from aware_amd.utils.models import load
    det, ys, bits, O = embedded
    trimmed = [y[256:] for y in ys]
    np.testing.assert_array_equal(np.asarray(detect_watermark(trimmed[0], 16000, det, sync_search=8)).reshape(-1)[:20], bits[0])
    got = detect_watermark_batch(trimmed, 16000, det, sync_search=8)
    np.testing.assert_array_equal(np.stack([np.asarray(g).reshape(-1)[:20] for g in got]), bits)
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        card = yaml.safe_load(f)
    card["sync_search"] = 8
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    _, searching = load(str(p))
    assert searching.sync_search == 8
    np.testing.assert_array_equal(np.asarray(detect_watermark(trimmed[1], 16000, searching)).reshape(-1)[:20], bits[1])
    stereo = np.column_stack([trimmed[0][:15000], trimmed[0][:15000]])
    np.testing.assert_array_equal(np.asarray(detect_watermark(stereo, 16000, searching)).reshape(-1)[:20], bits[0])
