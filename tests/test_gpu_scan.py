"""Scanning long recordings (EXTENSION) on the device: the two kernels of csrc/scan_kernels.hip
(aware_scan_select, aware_scan_segments) alone against the numpy restatement of detection/sync.py, on a ragged batch that
crosses the run scan's chunk of 256 windows and its carry; and the scan end to end: clips embedded on the device, spliced into
unmarked hosts, found again through AWAREDetector.scan and the service call.

Run on the MI355X box:  python -m pytest tests/test_gpu_scan.py -m gpu -q -s"""
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, make_clip
from test_scan_host import AT, ber, ragged_case, run_tuples, splice

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 255, 256, 257, 1025)
SENTINEL = -7


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


# ---- 1. the kernels alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sync,L,centre,max_flip,max_segments", [(1, 512, 0.0, 128, 400), (8, 20, 0.0, 5, 16), (64, 1, 0.5, 0, 16),
                                                                   (8, 64, 0.5, 16, 400), (64, 65, 0.0, 16, 7)])
def test_scan_kernels_match_the_restatement(rt, S, n_sync, L, centre, max_flip, max_segments):
    """Files of 1, 2, 255, 256, 257 and 1025 windows in one batch.  The case keeps every two confidences that a rule compares
    1e-5 apart or more, except the equal rows it puts in on purpose, so every integer is the restatement's; win_conf is
    aware_sync_select's bit for bit; the segment values are held within four times the distance between the float32 and the
    float64 restatement on the same input, a distance worked out here and printed."""
    values, off = ragged_case(n_sync, L, 2000 + 7 * L + n_sync, COUNTS, centre)
    W, B = off[-1], len(off) - 1
    dev = torch.from_numpy(values).cuda()
    out, view, conf, bits = rt.scan_select(dev, off, n_sync, centre)
    sel = rt.sync_select(dev, n_sync, centre)
    assert torch.equal(conf, sel[2]) and torch.equal(view, sel[1]) and torch.equal(out, sel[0])      # bit for bit
    r_out, r_view, r_conf, r_bits = S.scan_select(values, off, n_sync, centre)
    assert np.array_equal(view.cpu().numpy(), r_view)
    assert np.array_equal(out.cpu().numpy(), r_out)                                                  # the chosen rows
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), S.pack_bits(r_bits))
    print(f"n_sync {n_sync} L {L}: win_conf against numpy's summation order: max |diff| "
          f"{float(np.max(np.abs(conf.cpu().numpy() - r_conf))):.3e}")
    assert np.max(np.abs(conf.cpu().numpy() - r_conf)) < 1e-6          # another summation order; the case's gaps are 1e-5

    fill = {k: torch.full((B, max_segments), SENTINEL, dtype=torch.int32, device="cuda") for k in ("first", "last", "peak", "view")}
    fill.update(n_seg=torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda"),
                confidence=torch.full((B, max_segments), float(SENTINEL), dtype=torch.float32, device="cuda"),
                values=torch.full((B, max_segments, L), float(SENTINEL), dtype=torch.float32, device="cuda"))
    seg = rt.scan_segments(conf, view, out, bits, off, centre, 0.06, max_flip, max_segments, out=fill)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in seg.items()}
    # the restatement on the same input: the device's confidences and rows
    c_h, v_h, view_h = conf.cpu().numpy(), out.cpu().numpy(), view.cpu().numpy()
    f32 = S.scan_segments(c_h, v_h, off, centre, 0.06, max_flip, max_segments, view=view_h)
    f64 = S.scan_segments(c_h, v_h, off, centre, 0.06, max_flip, max_segments, view=view_h, dtype=np.float64)
    assert run_tuples(f32) == run_tuples(S.scan_segments(r_conf, r_out, off, centre, 0.06, max_flip, max_segments))
    assert got["n_seg"].tolist() == [count for count, _ in f32]
    distance = max([float(np.max(np.abs(a["values"] - b["values"]))) for (_, sa), (_, sb) in zip(f32, f64) for a, b in zip(sa, sb)])
    worst = 0.0
    for b, (count, segs) in enumerate(f32):
        assert len(segs) == min(count, max_segments)
        for r, s in enumerate(segs):
            assert (got["first"][b, r], got["last"][b, r], got["peak"][b, r], got["view"][b, r]) == (
                s["first"], s["last"], s["peak"], s["view"]), (b, r)
            assert got["confidence"][b, r] == np.float32(s["confidence"])
            worst = max(worst, float(np.max(np.abs(got["values"][b, r] - f64[b][1][r]["values"]))))
        for k in ("first", "last", "peak", "view", "confidence", "values"):
            assert (got[k][b, len(segs):] == SENTINEL).all(), (k, b)          # slots beyond the file's runs are untouched
    print(f"    runs per file {[count for count, _ in f32]}; segment values: float32 restatement against float64 {distance:.3e}, "
          f"device against float64 {worst:.3e}")
    assert worst <= 4.0 * distance
    assert max(count for count, _ in f32) > max_segments or max_segments >= 400       # the case cuts where it means to


def test_scan_entry_points_refuse_bad_arguments(rt):
    v = torch.zeros((6, 20), device="cuda")
    for off, n in (([0, 4], 2), ([1, 3], 2), ([0, 3, 2, 3], 2), ([0, 3], 65), ([0, 0], 2)):
        with pytest.raises(ValueError, match="scan_select"):
            rt.scan_select(v, off, n)
    with pytest.raises(ValueError, match="scan_select"):
        rt.scan_select(torch.zeros((3, 513), device="cuda"), [0, 3], 1)
    out, view, conf, bits = rt.scan_select(v, [0, 3], 2)
    for kw in ({"max_segments": 0}, {"max_flip": -1}, {"min_confidence": float("nan")}):
        args = {"centre": 0.0, "min_confidence": 0.06, "max_flip": 5, "max_segments": 4, **kw}
        with pytest.raises(ValueError, match="scan_segments"):
            rt.scan_segments(conf, view, out, bits, [0, 3], **args)
    with pytest.raises(ValueError, match="scan_segments"):
        rt.scan_segments(conf, view, out, bits, [0, 2], 0.0, 0.06, 5, 4)


# ---- 2. the scan end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spliced(rt):
    """Two 1 s clips embedded plainly on the device, 400 steps, each inside 9 s of unmarked audio at sample 37 123; a third
    file of 9 s unmarked."""
    from oracle import aware_oracle as O
    from aware_amd.utils.models import load
    emb, det = load()
    pairs = [make_clip(s, 16000) for s in range(2)]
    clips, bits = [p[0] for p in pairs], np.stack([p[1] for p in pairs])
    wm = np.stack([O.bits_to_bipolar(b) for b in bits]).astype(np.float32)
    ys = [o.cpu().numpy() for o in emb.embed_batch(clips, 16000, wm)]
    files = [splice(ys[k], 144000, 100 + k) for k in (0, 1)]
    rng = np.random.default_rng(103)
    files.append((rng.standard_normal(144000) * np.sqrt(np.mean(ys[0].astype(np.float64) ** 2))).astype(np.float32))
    spans, profiles = det.scan(files, 16000, return_profile=True)
    return det, ys, bits, files, spans, profiles


def crops_read(det, files, profiles, S, n=8):
    """Per file, detect_batch's plain read of the crop that every window chose: its own copy of the samples, no offsets.  The
    crops of all views of all windows go in one call, the scan's own batch (a batch of another size or of other lengths may take
    another conv pipe, whose values differ in the last bits)."""
    offs = S.sync_offsets(n)
    crops = [f[s + e:s + e + p["length"]] for f, p in zip(files, profiles) for s in p["starts"] for e in offs]
    vals = det.detect_batch(crops, 16000, sync_search=0).cpu().numpy()
    out, at = [], 0
    for p in profiles:
        rows = vals[at:at + n * len(p["starts"])].reshape(len(p["starts"]), n, -1)
        out.append(rows[np.arange(len(p["starts"])), p["win_view"]])
        at += n * len(p["starts"])
    return out


def test_scan_finds_the_spliced_clips(spliced, S):
    det, ys, bits, files, spans, profiles = spliced
    for k in (0, 1):
        print(f"file {k}: " + "; ".join(f"span {s['start']}..{s['end']} peak {s['peak']} confidence {s['confidence']:.4f} BER "
                                        f"{ber(s['values'], bits[k]):.0f} %" for s in spans[k])
              + f"; largest win_conf elsewhere {np.sort(profiles[k]['win_conf'])[-6]:.4f}")
        assert len(spans[k]) == 1 and profiles[k]["n_segments"] == 1
        s = spans[k][0]
        assert ber(s["values"], bits[k]) == 0.0
        assert abs(s["peak"] - AT) <= 64
        assert s["start"] <= AT and s["end"] >= AT + len(ys[k]) and s["windows"][0] <= s["windows"][1]
        prof = profiles[k]
        peak = int(np.argmax(prof["win_conf"]))
        assert prof["starts"][peak] + S.sync_offsets(8)[int(prof["win_view"][peak])] == s["peak"]
        assert float(prof["win_conf"][peak]) == s["confidence"] and s["windows"][0] <= peak <= s["windows"][1]
    # every window's row, the peaks' among them, is detect_batch's read of that crop, bit for bit
    for k, rows in enumerate(crops_read(det, files, profiles, S)):
        assert np.array_equal(profiles[k]["win_values"], rows), k
    print(f"unmarked file: largest win_conf {profiles[2]['win_conf'].max():.4f}")
    assert spans[2] == [] and profiles[2]["n_segments"] == 0
    assert len(profiles[2]["starts"]) == 33 and profiles[2]["length"] == 16000


def test_scan_in_small_chunks_is_the_same_scan(spliced):
    """792 rows in calls of 100: eight calls, cut inside windows and files.  A batch of another size may take another conv pipe
    (test_gpu_sync_search.py), so bit equality is asked of the spans, windows and views, and the values are held to 1e-4: the
    bound smoke() holds any detect call to against the oracle, whatever its pipe, so two reads of one crop that both pass it
    are 2e-4 apart at most, and half of that is asked.  A row assigned to the wrong window at a chunk's edge would differ by
    about the size of an unmarked value, 0.02 or more."""
    det, ys, bits, files, spans, profiles = spliced
    assert det.scan_rows_per_call == 4096
    det.scan_rows_per_call = 100
    try:
        chunked, prof = det.scan(files, 16000, return_profile=True)
    finally:
        det.scan_rows_per_call = 4096
    worst = 0.0
    for x, y in zip(chunked, spans):
        assert len(x) == len(y)
        for s, t in zip(x, y):
            assert all(s[k] == t[k] for k in ("start", "end", "peak", "windows"))
            worst = max(worst, float(np.max(np.abs(s["values"] - t["values"]))), abs(s["confidence"] - t["confidence"]))
    for a, b in zip(prof, profiles):
        assert a["starts"] == b["starts"] and np.array_equal(a["win_view"], b["win_view"]) and a["n_segments"] == b["n_segments"]
        worst = max(worst, float(np.max(np.abs(a["win_conf"] - b["win_conf"]))), float(np.max(np.abs(a["win_values"] - b["win_values"]))))
    print(f"calls of 100 rows against one call: largest difference of a value or confidence {worst:.3e}")
    assert worst < 1e-4


def test_scan_short_files(spliced, S):
    """One window where the file is shorter than a window and the largest offset; refusal, by the file's index, where the
    shortest view would have 512 samples or fewer (at 8 views the offsets take 448 samples, so that is any file of up to 960)."""
    det, ys, bits, files, spans, profiles = spliced
    short = files[0][AT:AT + 448 + 700]                          # views of 700 samples
    found, prof = det.scan([files[2], short], 16000, return_profile=True)
    assert prof[1]["starts"] == [0] and prof[1]["length"] == 700 and len(prof[1]["win_conf"]) == 1
    assert len(prof[0]["starts"]) == 33 and found[0] == []
    for k, rows in enumerate(crops_read(det, [files[2], short], prof, S)):
        assert np.array_equal(prof[k]["win_values"], rows), k
    for n in (520, 700, 960):
        with pytest.raises(ValueError, match=rf"file 1 has {n} samples"):
            det.scan([files[2], files[0][:n]], 16000)
    prof = det.scan([files[0][:1000]], 16000, sync_search=2, return_profile=True)[1][0]       # the offsets take 256 samples
    assert prof["starts"] == [0] and prof["length"] == 744
    # one view per window (an explicit sync_search of 0 or 1): no offsets, so a 700-sample file is one window of 700
    for n in (1, 0):
        one = det.scan([files[0][AT:AT + 700]], 16000, sync_search=n, return_profile=True)[1][0]
        assert one["starts"] == [0] and one["length"] == 700 and one["win_view"].tolist() == [0]
    plain = det.detect_batch([files[0][AT:AT + 700]], 16000, sync_search=0).cpu().numpy()[0]
    assert np.array_equal(one["win_values"][0], plain)                                        # the same batch of one row
    with pytest.raises(ValueError, match="file 0 has 520 samples"):
        det.scan([files[0][:520]], 16000, sync_search=2)
    with pytest.raises(ValueError, match="hop_samples"):
        det.scan(files[:1], 16000, hop_samples=1000)
    with pytest.raises(ValueError, match="speed_search"):
        det.speed_search = S.check_speed_search(2.0)
        try:
            det.scan(files[:1], 16000)
        finally:
            det.speed_search = None


def test_the_service_and_the_card_key(spliced, tmp_path):
    from aware_amd import service
    from aware_amd.utils.models import load
    det, ys, bits, files, spans, profiles = spliced
    found = service.scan_watermark(files[0], 16000, det)
    assert len(found) == 1 and np.array_equal(np.asarray(found[0]["payload"]), bits[0])
    assert (found[0]["start"], found[0]["end"], found[0]["peak"]) == tuple(spans[0][0][k] for k in ("start", "end", "peak"))
    batch = service.scan_watermark_batch(files, 16000, det)
    assert [len(f) for f in batch] == [1, 1, 0] and np.array_equal(np.asarray(batch[1][0]["payload"]), bits[1])
    stereo = service.scan_watermark(np.column_stack([files[2], files[1]]), 16000, det)
    assert len(stereo) == 1 and np.array_equal(np.asarray(stereo[0]["payload"]), bits[1])
    same = service.scan_watermark(np.column_stack([files[0], files[0]]), 16000, det)          # one span heard twice
    assert len(same) == 1 and np.array_equal(np.asarray(same[0]["payload"]), bits[0])
    both = service.scan_watermark(np.column_stack([files[0], files[1]]), 16000, det)          # two payloads at one place
    assert len(both) == 2 and sorted(tuple(np.asarray(f["payload"])) for f in both) == sorted(tuple(b) for b in bits)
    assert service.scan_watermark(files[0], 16000, det, min_confidence=0.5) == []
    with pytest.raises(ValueError, match="16000"):
        service.scan_watermark(files[0], 8000, det)
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        card = yaml.safe_load(f)
    card["scan"] = {"min_confidence": 0.5, "max_segments": 2}
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    _, strict = load(str(p))
    assert strict.scan_defaults["min_confidence"] == 0.5 and strict.scan(files[:1], 16000) == [[]]
    assert len(strict.scan(files[:1], 16000, min_confidence=0.06)[0]) == 1
