"""CPU tests of the scan of long recordings (no GPU): the window geometry, the selection and the runs of
aware_amd/detection/sync.py on hand-made values, the parameter checks, the card key, the ABI's refusals, the kernel bodies
compiled for the host (tests/host_sim/scan_check.cpp) against the restatement, and the value claims on the CPU oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, make_clip
from oracle import aware_oracle as O
from aware_amd.detection import sync

F32 = np.float32


# ---- 1. the windows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sync", [1, 8, 64])
def test_scan_windows(n_sync):
    e_max = sync.sync_offsets(n_sync)[-1]
    assert e_max == {1: 0, 8: 448, 64: 504}[n_sync]
    window, hop = 16000, 4096
    # on the grid: the last window ends on the file's last sample, no tail window
    n = 3 * hop + window + e_max
    assert sync.scan_windows(n, window, hop, n_sync) == ([0, hop, 2 * hop, 3 * hop], window)
    # one sample more: a tail window, one sample off the grid
    starts, length = sync.scan_windows(n + 1, window, hop, n_sync)
    assert (starts, length) == ([0, hop, 2 * hop, 3 * hop, 3 * hop + 1], window)
    assert all(s + e_max + length <= n + 1 for s in starts) and starts[-1] + e_max + length == n + 1
    # one sample fewer: the grid loses its last window and the tail takes its place
    assert sync.scan_windows(n - 1, window, hop, n_sync)[0] == [0, hop, 2 * hop, 3 * hop - 1]
    # exactly one window, and files shorter than that: one window of what is left after the largest offset
    assert sync.scan_windows(window + e_max, window, hop, n_sync) == ([0], window)
    assert sync.scan_windows(window + e_max - 1, window, hop, n_sync) == ([0], window - 1)
    assert sync.scan_windows(513 + e_max, window, hop, n_sync) == ([0], 513)
    # refused, by the file's index
    with pytest.raises(ValueError, match=r"file 3 has \d+ samples"):
        sync.scan_windows(512 + e_max, window, hop, n_sync, index=3)
    with pytest.raises(ValueError, match="hop_samples"):
        sync.scan_windows(n, window, 4000, n_sync)
    with pytest.raises(ValueError, match="hop_samples"):
        sync.scan_windows(n, window, 0, n_sync)
    with pytest.raises(ValueError, match="window"):
        sync.scan_windows(n, 512, hop, n_sync)


def test_scan_windows_the_issue_s_files():
    """9 s at the defaults: the windows the value claims below count."""
    starts, length = sync.scan_windows(144000, 16000, 4096, 8)
    assert length == 16000 and starts[:3] == [0, 4096, 8192] and starts[-1] == 144000 - 16000 - 448 and len(starts) == 33
    assert len(sync.scan_windows(320000, 16000, 4096, 8)[0]) == 76              # the 20 s file: 608 rows


# ---- 2. selection and runs on hand-made values ---------------------------------------------------------------------------------------
def rows(conf, bits, centre=0.0):
    """A row per window: value centre +- conf[w] with the sign of bits[w][l]; its confidence is conf[w]."""
    conf, bits = np.asarray(conf, dtype=F32), np.asarray(bits, dtype=bool)
    return (F32(centre) + np.where(bits, 1, -1).astype(F32) * conf[:, None]).astype(F32)


def run_tuples(result):
    return [(count, [(s["first"], s["last"], s["peak"]) for s in segs]) for count, segs in result]


def test_scan_select_hand_made():
    L, n = 20, 4
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2, (3 * n, L)).astype(bool)
    conf = np.array([0.1, 0.3, 0.3, 0.2,        # a tie of equal rows: the smaller view
                     0.5, 0.1, 0.1, 0.9,        # a clear winner, last
                     0.2, 0.2, 0.2, 0.2], dtype=F32)
    v = rows(conf, bits)
    v[2] = v[1]
    v[9:12] = v[8]
    v[5, 3] = np.nan                            # a NaN row never wins
    out, view, c, b = sync.scan_select(v, [0, 1, 3], n, 0.0)
    assert view.tolist() == [1, 3, 0] and view.dtype == np.int32
    assert np.array_equal(out, v[[1, 7, 8]]) and out.dtype == F32
    ref = sync.sync_select(np.nan_to_num(v, nan=0.0), n, 0.0)
    assert np.array_equal(c, ref[2]) and np.array_equal(view, ref[1])       # sync_select's order and precision
    assert np.array_equal(b, out > 0)
    # all rows of a window NaN: view 0, confidence -1 (as aware_sync_select), so never marked
    v[4:8] = np.nan
    out, view, c, b = sync.scan_select(v, [0, 3], n, 0.0)
    assert view[1] == 0 and c[1] == -1.0 and not b[1].any()
    assert run_tuples(sync.scan_segments(c, out, [0, 3], 0.0, 0.06, 20, 4)) == [(2, [(0, 0, 0), (2, 2, 2)])]
    # centre 0.5: confidences and bits about the centre
    v = rows([0.2, 0.4], bits[:2], centre=0.5)
    out, view, c, b = sync.scan_select(v, [0, 1], 2, 0.5)
    assert view.tolist() == [1] and abs(float(c[0]) - 0.4) < 1e-6 and np.array_equal(b[0], bits[1])
    with pytest.raises(ValueError, match="scan_select"):
        sync.scan_select(v, [0, 2], 2, 0.5)


def test_pack_bits():
    rng = np.random.default_rng(1)
    for L in (1, 20, 32, 33, 64, 65, 512):
        bits = rng.integers(0, 2, (3, L)).astype(bool)
        words = sync.pack_bits(bits)
        assert words.shape == (3, (L + 31) // 32) and words.dtype == np.uint32
        for l in range(L):
            assert np.array_equal((words[:, l // 32] >> np.uint32(l % 32)) & 1, bits[:, l].astype(np.uint32))
        if L % 32:
            assert not (words[:, -1] >> np.uint32(L % 32)).any()


@pytest.mark.parametrize("centre", [0.0, 0.5])
@pytest.mark.parametrize("L", [1, 20, 512])
def test_scan_segments_hand_made(L, centre):
    rng = np.random.default_rng(L)
    base = rng.integers(0, 2, L).astype(bool)
    thr = 0.06

    def seg(conf, bits, off, max_flip=0, max_segments=8):
        return sync.scan_segments(np.asarray(conf, dtype=F32), rows(conf, bits, centre), off, centre, thr, max_flip, max_segments)

    # a run touching the first window and one touching the last, two files
    conf = [0.2, 0.3, 0.01, 0.01, 0.1, 0.25, 0.02, 0.4]
    res = seg(conf, [base] * 8, [0, 6, 8])
    assert run_tuples(res) == [(2, [(0, 1, 1), (4, 5, 5)]), (1, [(1, 1, 1)])]
    assert res[0][1][0]["confidence"] == float(F32(0.3)) and res[1][1][0]["confidence"] == float(F32(0.4))
    # all marked, none marked
    assert run_tuples(seg([0.2] * 5, [base] * 5, [0, 5])) == [(1, [(0, 4, 0)])]        # a tie on the peak: the smaller index
    assert run_tuples(seg([0.059] * 5, [base] * 5, [0, 5])) == [(0, [])]
    assert run_tuples(seg([0.06] * 2, [base] * 2, [0, 2])) == [(1, [(0, 1, 0)])]       # the threshold itself is marked
    # NaN: never marked, and it parts the run
    res = sync.scan_segments(np.array([0.2, np.nan, 0.2], dtype=F32), rows([0.2] * 3, [base] * 3, centre), [0, 3], centre, thr, 0, 8)
    assert run_tuples(res) == [(2, [(0, 0, 0), (2, 2, 2)])]
    # more runs than max_segments: the first ones, and the true count
    conf = [0.2, 0.0] * 5
    assert run_tuples(seg(conf, [base] * 10, [0, 10], max_segments=3)) == [(5, [(0, 0, 0), (2, 2, 2), (4, 4, 4)])]
    # the values: one window gives its row back (to rounding), a run the weighted mean in float32 and ascending order
    conf = np.array([0.1, 0.3, 0.2], dtype=F32)
    V = (F32(centre) + rng.standard_normal((3, L)).astype(F32) * F32(0.2)).astype(F32)
    res = sync.scan_segments(conf, V, [0, 3], centre, -1.0, L, 8)
    assert run_tuples(res) == [(1, [(0, 2, 1)])]
    num, den = np.zeros(L, dtype=F32), F32(0)
    for w in range(3):
        num = num + conf[w] * (V[w] - F32(centre))
        den = den + conf[w]
    assert np.array_equal(res[0][1][0]["values"], F32(centre) + num / den) and res[0][1][0]["values"].dtype == F32
    exact = sync.scan_segments(conf, V, [0, 3], centre, -1.0, L, 8, dtype=np.float64)[0][1][0]["values"]
    assert exact.dtype == np.float64 and np.max(np.abs(exact - res[0][1][0]["values"])) < 1e-6
    # `view` is the peak window's
    assert sync.scan_segments(conf, V, [0, 3], centre, -1.0, L, 8, view=np.array([5, 6, 7]))[0][1][0]["view"] == 6


@pytest.mark.parametrize("L,flips", [(20, 5), (64, 16), (65, 1), (512, 128)])
def test_scan_segments_flip_rule(L, flips):
    """Two runs separated only by the flip rule: max_flip exactly met joins them, exceeded by one parts them."""
    rng = np.random.default_rng(L)
    a = rng.integers(0, 2, L).astype(bool)
    b = a.copy()
    b[rng.permutation(L)[:flips]] ^= True
    conf = np.array([0.2, 0.3, 0.25, 0.2], dtype=F32)
    V = rows(conf, [a, a, b, b])
    assert run_tuples(sync.scan_segments(conf, V, [0, 4], 0.0, 0.06, flips, 8)) == [(1, [(0, 3, 1)])]
    assert run_tuples(sync.scan_segments(conf, V, [0, 4], 0.0, 0.06, flips - 1, 8)) == [(2, [(0, 1, 1), (2, 3, 2)])]


# ---- 3. parameters, card, ABI ------------------------------------------------------------------------------------------------------
def test_check_scan():
    d = sync.check_scan()
    assert d == {"window_seconds": 1.0, "hop_samples": 4096, "min_confidence": 0.06, "max_segments": 16, "max_flip": None,
                 "window": 16000}
    assert sync.check_scan(0.5, 512, -0.1, 1, 0, 16000)["window"] == 8000
    for key, kwargs in (("window_seconds", {"window_seconds": 0.032}), ("window_seconds", {"window_seconds": float("nan")}),
                        ("window_seconds", {"window_seconds": "1"}), ("window_seconds", {"window_seconds": -1.0}),
                        ("window_seconds", {"window_seconds": 1e9}), ("window_seconds", {"window_seconds": True}),
                        ("hop_samples", {"hop_samples": 4000}), ("hop_samples", {"hop_samples": 0}),
                        ("hop_samples", {"hop_samples": 4096.0}), ("hop_samples", {"hop_samples": -512}),
                        ("min_confidence", {"min_confidence": float("inf")}), ("min_confidence", {"min_confidence": None}),
                        ("max_segments", {"max_segments": 0}), ("max_segments", {"max_segments": 1.5}),
                        ("max_flip", {"max_flip": -1}), ("max_flip", {"max_flip": 2.0})):
        with pytest.raises(ValueError, match=key):
            sync.check_scan(**kwargs)
    assert sync.check_scan_card(None) == {k: d[k] for k in sync.SCAN_KEYS}
    assert sync.check_scan_card({"hop_samples": 2048})["hop_samples"] == 2048
    with pytest.raises(ValueError, match="max_flip"):
        sync.check_scan_card({"max_flip": 3})                  # not a card key
    with pytest.raises(ValueError, match="scan"):
        sync.check_scan_card([1.0])


def test_card_key_reaches_the_detector(tmp_path):
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        text = f.read()
    assert "# scan: {window_seconds: 1.0, hop_samples: 4096, min_confidence: 0.06, max_segments: 16}" in text
    card = yaml.safe_load(text)
    assert "scan" not in card                                  # the committed card keeps its behaviour
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    assert load(str(p))[1].scan_defaults == {"window_seconds": 1.0, "hop_samples": 4096, "min_confidence": 0.06, "max_segments": 16}
    card["scan"] = {"window_seconds": 0.5, "hop_samples": 2048, "min_confidence": 0.1, "max_segments": 4}
    p.write_text(yaml.safe_dump(card))
    assert load(str(p))[1].scan_defaults == card["scan"]
    card["scan"] = {"min_confidence": 0.08}
    p.write_text(yaml.safe_dump(card))
    assert load(str(p))[1].scan_defaults == {"window_seconds": 1.0, "hop_samples": 4096, "min_confidence": 0.08, "max_segments": 16}
    for bad in ({"hop_samples": 1000}, {"window_seconds": 0.01}, {"max_segments": 0}, {"min_confidence": "high"}, {"hop": 4096}, 3):
        card["scan"] = bad
        p.write_text(yaml.safe_dump(card))
        assert load(str(p)) is None, bad


def test_scan_refuses_speed_search_by_name():
    from aware_amd.utils.models import load
    det = load()[1]
    det.speed_search = sync.check_speed_search(2.0)
    with pytest.raises(ValueError, match="speed_search"):
        det.scan([np.zeros(16000, dtype=F32)], 16000)


def test_stereo_rule_keeps_adjacent_payloads():
    """Two adjacent clips scan to two overlapping spans (32768..56960 and 49152..73344).  Whichever
    channels hold them, both payloads come back: a span is only replaced by its counterpart in the other channel, the span it
    overlaps most (mutually) and whose bits differ from its own in at most max_flip places."""
    from aware_amd.service.detect import _scan_stereo
    rng = np.random.default_rng(5)
    pa = rng.integers(0, 2, 20).astype(bool)
    pb = pa.copy()
    pb[:11] ^= True                                             # 55 % of the bits, as measured between seeds 0 and 1

    def span(start, end, confidence, payload, tag):
        return {"start": start, "end": end, "peak": start + 4352, "confidence": confidence, "tag": tag,
                "values": np.where(payload, confidence, -confidence).astype(F32)}

    def stereo(left, right, max_flip=5):
        return [s["tag"] for s in _scan_stereo(left, right, max_flip)]

    a, b = span(32768, 56960, 0.241, pa, "a"), span(49152, 73344, 0.212, pb, "b")
    assert stereo([a, b], []) == ["a", "b"]                     # only left
    assert stereo([], [a, b]) == ["a", "b"]                     # only right
    assert stereo([], []) == []
    assert stereo([a, b], [dict(a, tag="ra"), dict(b, tag="rb")]) == ["a", "b"]               # both, equal: the left ones
    louder = [span(32768, 56960, 0.25, pa, "ra"), span(49152, 73344, 0.22, pb, "rb")]
    assert stereo([a, b], louder) == ["ra", "rb"]               # both, right more confident: each replaces its counterpart
    assert stereo(louder, [a, b]) == ["ra", "rb"]
    assert stereo([a, b], [louder[0], span(49152, 73344, 0.1, pb, "rb")]) == ["ra", "b"]
    assert stereo([a], [b]) == ["a", "b"] and stereo([b], [a]) == ["a", "b"]                  # one clip per channel: two payloads
    few = pa.copy()
    few[:5] ^= True                                             # max_flip exactly met: one span heard twice
    assert stereo([a], [span(36864, 56960, 0.3, few, "r")]) == ["r"]
    few[5] ^= True                                              # exceeded by one: two payloads
    assert stereo([a], [span(36864, 56960, 0.3, few, "r")]) == ["a", "r"]
    # one long span against two: its counterpart is the one it overlaps most, the other stays
    long = span(32768, 73344, 0.3, pa, "long")
    assert stereo([long], [a, b]) == ["long", "b"] and stereo([a, b], [long]) == ["long", "b"]
    assert stereo([a], [span(100000, 124192, 0.1, pa, "far")]) == ["a", "far"]                # no overlap: both
    assert stereo([a], [dict(a, tag="r")], max_flip=0) == ["a"]


def test_abi_symbols_and_bad_arguments():
    from aware_amd import _lib, runtime as rt, service
    lib = _lib.load_library()
    for name in ("aware_scan_select", "aware_scan_segments"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "scan_kernels.hip" in _lib.SOURCES
    assert lib.aware_version() == 350
    with open(os.path.join(ROOT, "include", "aware_hip.h")) as f:
        hdr = f.read()
    assert "int aware_scan_select(" in hdr and "int aware_scan_segments(" in hdr
    assert callable(rt.scan_select) and callable(rt.scan_segments)
    assert callable(service.scan_watermark) and callable(service.scan_watermark_batch)
    p = C.c_void_p(256)                                         # never dereferenced: every call below is refused
    q = C.c_void_p(512)
    off = (C.c_int * 3)(0, 2, 5)
    down = (C.c_int * 3)(0, 3, 2)
    late = (C.c_int * 3)(1, 2, 5)
    none = (C.c_int * 3)(0, 0, 0)

    def select(values=p, win_off=off, B=2, n=8, L=20, centre=0.0, conf=q, view=q, out=q, bits=q):
        return lib.aware_scan_select(values, win_off, B, n, L, centre, conf, view, out, bits, None)

    assert select(values=None) == -1 and select(win_off=None) == -1 and select(conf=None) == -1 and select(view=None) == -1
    assert select(out=None) == -1 and select(bits=None) == -1 and select(out=p) == -1
    for kw in ({"B": 0}, {"B": -1}, {"n": 0}, {"n": 65}, {"L": 0}, {"L": 513}, {"centre": float("nan")}, {"win_off": down},
               {"win_off": late}, {"win_off": none}):
        assert select(**kw) == -1, kw

    def segments(ptrs=None, win_off=off, B=2, L=20, centre=0.0, min_conf=0.06, max_flip=5, max_segments=16):
        a = [p, p, p, p, win_off, p, q, q, q, q, q, q, q] if ptrs is None else ptrs
        return lib.aware_scan_segments(a[0], a[1], a[2], a[3], a[4], a[5], B, L, centre, min_conf, max_flip, max_segments,
                                       a[6], a[7], a[8], a[9], a[10], a[11], a[12], None)

    for i in range(13):                                         # each pointer in turn
        a = [p, p, p, p, off, p, q, q, q, q, q, q, q]
        a[i] = None
        assert segments(ptrs=a) == -1, i
    for kw in ({"B": 0}, {"L": 0}, {"L": 513}, {"centre": float("inf")}, {"min_conf": float("nan")}, {"min_conf": float("inf")},
               {"max_flip": -1}, {"max_segments": 0}, {"win_off": down}, {"win_off": late}, {"win_off": none}):
        assert segments(**kw) == -1, kw


# ---- 4. the kernel bodies on the host ----------------------------------------------------------------------------------------------
def ragged_case(n_sync, L, seed, counts=(1, 2, 255, 256, 257, 1025), centre=0.0):
    """values [W * n_sync, L] for files of `counts` windows, drawn so that no two confidences the rules compare are closer
    than 1e-5 (the confidences of a window's views, of a run's windows, and the threshold 0.06), except the equal rows put in
    on purpose: every 7th window repeats its best view (a tie between views), every 11th repeats the window before it (a tie
    on a run's peak).  Runs of marked windows of mixed lengths; the bits of a run drift by few flips, a new payload parts it."""
    rng = np.random.default_rng(seed)
    W = int(sum(counts))
    marked = np.zeros(W, dtype=bool)
    w = 0
    while w < W:
        run = int(rng.integers(1, 40))
        marked[w:w + run] = rng.random() < 0.6
        w += run
    marked[[0, W - 1]] = True
    # the best view of window w reads base[w], on a grid of 2e-5 and different for every window: 0.07 to 0.106 where marked,
    # 0.01 to 0.046 where not; its other views read half of that less 2e-5 times their rank
    base = np.where(marked, 0.07, 0.01) + 2e-5 * rng.permutation(W)
    rank = np.argsort(rng.random((W, n_sync)), axis=1)
    conf = np.where(rank == 0, base[:, None], 0.5 * base[:, None] - 2e-5 * rank).astype(F32)
    bits = np.zeros((W, L), dtype=bool)
    cur = rng.integers(0, 2, L).astype(bool)
    for w in range(W):
        r = rng.random()
        if r < 0.1:
            cur = rng.integers(0, 2, L).astype(bool)             # a new payload
        elif r < 0.5 and L > 1:
            cur = cur.copy()
            cur[rng.integers(0, L, int(rng.integers(1, max(2, L // 8))))] ^= True
        bits[w] = cur
    # magnitudes: pairs (2 k, 2 k + 1) of a row move apart by the same amount, so the mean stays while the sums have rounding
    # to disagree about
    mag = np.repeat(conf[:, :, None], L, axis=2).astype(np.float64)
    d = conf[:, :, None] * 0.3 * rng.random((W, n_sync, L // 2))
    mag[:, :, 0:2 * (L // 2):2] += d
    mag[:, :, 1:2 * (L // 2):2] -= d
    v = np.empty((W, n_sync, L), dtype=F32)
    for j in range(n_sync):
        flip = rng.random((W, L)) < (0.0 if j == 0 else 0.2)
        v[:, j] = (centre + np.where(bits ^ flip, 1.0, -1.0) * mag[:, j]).astype(F32)
    best = np.argmax(np.abs(v - F32(centre)).mean(axis=-1, dtype=F32), axis=1)
    for w in range(0, W, 7):
        if n_sync > 1:
            v[w, (best[w] + 1) % n_sync] = v[w, best[w]]
    off = np.concatenate([[0], np.cumsum(counts)]).tolist()
    for w in range(11, W, 11):
        if w not in off:
            v[w] = v[w - 1]
    return v.reshape(W * n_sync, L), off


def restate(values, off, n_sync, centre, min_conf, max_flip, max_segments, dtype=F32):
    out, view, conf, bits = sync.scan_select(values, off, n_sync, centre)
    return out, view, conf, bits, sync.scan_segments(conf, out, off, centre, min_conf, max_flip, max_segments, view=view, dtype=dtype)


@pytest.fixture(scope="module")
def scan_check(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "host_sim", "scan_check.cpp")
    exe = str(tmp_path_factory.mktemp("scan") / "scan_check")
    subprocess.run(["c++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                   check=True)
    return exe


@pytest.mark.parametrize("n_sync,L,max_flip,max_segments", [(8, 20, 5, 16), (1, 65, 16, 3), (3, 512, 128, 400), (2, 1, 0, 16)])
def test_kernel_bodies_on_the_host(scan_check, tmp_path, n_sync, L, max_flip, max_segments):
    """The two kernel bodies, compiled for the host and run thread by thread under AddressSanitizer and UBSan, on the ragged
    case: every output equal to the restatement's, the float sums bit for bit (the host runs them unfused, as stated), and the
    slots beyond a file's runs untouched."""
    values, off = ragged_case(n_sync, L, 1000 + L)
    W, B, words = off[-1], len(off) - 1, (L + 31) // 32
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        np.array([B, n_sync, L, max_flip, max_segments], dtype=np.int32).tofile(f)
        np.array([0.0, 0.06], dtype=F32).tofile(f)
        np.array(off, dtype=np.int32).tofile(f)
        values.tofile(f)
    subprocess.run([scan_check, str(src), str(dst)], check=True)
    raw = np.fromfile(dst, dtype=np.int32)
    at = [0]

    def take(n):
        at[0] += n
        return raw[at[0] - n:at[0]]

    conf, view = take(W).view(F32), take(W)
    out, bits = take(W * L).view(F32).reshape(W, L), take(W * words).view(np.uint32).reshape(W, words)
    n_seg = take(B)
    S = max_segments
    first, last, peak, sview = (take(B * S).reshape(B, S) for _ in range(4))
    sconf, svalues = take(B * S).view(F32).reshape(B, S), take(B * S * L).view(F32).reshape(B, S, L)
    assert at[0] == raw.size
    r_out, r_view, r_conf, r_bits, r_seg = restate(values, off, n_sync, 0.0, 0.06, max_flip, S)
    assert np.array_equal(view, r_view) and np.array_equal(out, r_out) and np.array_equal(bits, sync.pack_bits(r_bits))
    assert np.max(np.abs(conf - r_conf)) < 1e-6                 # another summation order than numpy's
    assert [c for c, _ in r_seg] == n_seg.tolist()
    # the runs from the program's own confidences: then every float is the restatement's, bit for bit
    mine = sync.scan_segments(conf, out, off, 0.0, 0.06, max_flip, S, view=view)
    assert run_tuples(mine) == run_tuples(r_seg)
    sentinel = np.int32(-7)
    for b, (count, segs) in enumerate(mine):
        assert count > S or len(segs) == count
        for r, s in enumerate(segs):
            assert (first[b, r], last[b, r], peak[b, r], sview[b, r]) == (s["first"], s["last"], s["peak"], s["view"])
            assert sconf[b, r] == F32(s["confidence"]) and np.array_equal(svalues[b, r], s["values"])
        for a in (first, last, peak, sview, sconf.view(np.int32), svalues.view(np.int32)):
            assert (a[b, len(segs):] == sentinel).all()
    assert max(c for c, _ in mine) > 4 and any(s["last"] - s["first"] > 3 for _, segs in mine for s in segs)


# ---- 5. the value claims, on the CPU oracle ------------------------------------------------------------------------------------------
AT = 37123
MIN_CONFIDENCE, N_SYNC, WINDOW, HOP = 0.06, 8, 16000, 4096


def cpu_scan(plain, audio, min_confidence=MIN_CONFIDENCE, max_segments=16):
    """AWAREDetector.scan at the defaults, on the oracle's detector: (spans, profile) of one file."""
    starts, length = sync.scan_windows(len(audio), WINDOW, HOP, N_SYNC)
    offs = sync.sync_offsets(N_SYNC)
    crops = np.stack([audio[s + e:s + e + length] for s in starts for e in offs])
    vals = np.concatenate([plain.detect_raw(crops[i:i + 128]).numpy() for i in range(0, len(crops), 128)])
    off = [0, len(starts)]
    out, view, conf, _ = sync.scan_select(vals, off, N_SYNC, 0.0)
    count, segs = sync.scan_segments(conf, out, off, 0.0, min_confidence, vals.shape[1] // 4, max_segments, view=view)[0]
    spans = [{"start": starts[s["first"]], "end": starts[s["last"]] + length, "peak": starts[s["peak"]] + offs[s["view"]],
              "confidence": s["confidence"], "values": s["values"]} for s in segs]
    return spans, {"starts": starts, "length": length, "win_conf": conf, "win_view": view, "n_segments": count}


def splice(marked, total, seed, at=AT):
    """`marked` (one clip, or several back to back) inside unmarked Gaussian audio of `total` samples at its RMS."""
    marked = np.concatenate(marked) if isinstance(marked, (list, tuple)) else marked
    rng = np.random.default_rng(seed)
    host = (rng.standard_normal(total) * np.sqrt(np.mean(marked.astype(np.float64) ** 2))).astype(F32)
    host[at:at + len(marked)] = marked
    return host


def ber(values, bits):
    return O.ber_percent(O.decode_bits(values), bits)


@pytest.fixture(scope="module")
def scan_value_setup():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    plain = O.Embedder()
    bits = np.stack([make_clip(s, 16000)[1] for s in (0, 1)])
    wm = np.stack([O.bits_to_bipolar(b) for b in bits]).astype(F32)
    y1 = plain.embed(np.stack([make_clip(s, 16000)[0] for s in (0, 1)]), wm)[0].numpy()
    y3 = plain.embed(np.stack([make_clip(s, 48000)[0] for s in (0, 1)]), wm)[0].numpy()
    return plain, bits, y1, y3


def test_scan_finds_spliced_clips(scan_value_setup):
    """1 s marked inside 9 s and 3 s marked inside 11 s, seeds 0 and 1, at sample 37 123 of unmarked Gaussian hosts at the
    marked clip's RMS.  Measured with this restatement: DESIGN.md section 28."""
    plain, bits, y1, y3 = scan_value_setup
    whole, lo_marked = [], []
    for name, ys, total in (("1 s in 9 s", y1, 144000), ("3 s in 11 s", y3, 176000)):
        for k in (0, 1):
            audio = splice(ys[k], total, 100 + k)
            whole_values = plain.detect_raw(audio[None])[0].numpy()
            whole.append(ber(whole_values, bits[k]))
            spans, prof = cpu_scan(plain, audio)
            print(f"{name}, seed {k}: whole-file BER {whole[-1]:.0f} %, confidence {float(np.abs(whole_values).mean()):.4f}; "
                  + "; ".join(f"span {s['start']}..{s['end']} peak {s['peak']} confidence {s['confidence']:.4f} BER "
                              f"{ber(s['values'], bits[k]):.0f} %" for s in spans))
            assert len(spans) == 1 and prof["n_segments"] == 1
            assert ber(spans[0]["values"], bits[k]) == 0.0
            assert spans[0]["start"] <= AT + len(ys[k]) and spans[0]["end"] >= AT
            if len(ys[k]) < 20000:
                assert abs(spans[0]["peak"] - AT) <= 64
            offs = sync.sync_offsets(N_SYNC)
            begin = np.array(prof["starts"]) + np.array(offs)[prof["win_view"]]
            overlap = np.clip(np.minimum(begin + prof["length"], AT + len(ys[k])) - np.maximum(begin, AT), 0, None) / prof["length"]
            for lo, hi in ((0.4, 0.6), (0.7, 0.8), (0.9, 1.01)):
                sel = prof["win_conf"][(overlap >= lo) & (overlap < hi)]
                if len(sel):
                    print(f"    overlap {lo}..{hi}: win_conf {sel.min():.4f}..{sel.max():.4f} ({len(sel)} windows)")
            lo_marked.append(float(prof["win_conf"][overlap >= 0.9].min()))
    print(f"mean whole-file BER {np.mean(whole):.2f} %; smallest win_conf at overlap >= 0.9: {min(lo_marked):.4f}")
    assert np.mean(whole) >= 20.0
    assert MIN_CONFIDENCE < min(lo_marked)


def test_scan_parts_two_payloads(scan_value_setup):
    """Two 1 s clips with different payloads, back to back inside 10 s: two spans, each its own payload."""
    plain, bits, y1, _ = scan_value_setup
    spans, prof = cpu_scan(plain, splice([y1[0], y1[1]], 160000, 102))
    table = [[ber(s["values"], bits[k]) for k in (0, 1)] for s in spans]
    print("spans " + "; ".join(f"{s['start']}..{s['end']} confidence {s['confidence']:.4f}" for s in spans) + f"; BER % {table}")
    assert len(spans) == 2 and prof["n_segments"] == 2
    assert table[0][0] == 0.0 and table[1][1] == 0.0
    assert table[0][1] >= 25.0 and table[1][0] >= 25.0
    assert spans[0]["end"] > spans[0]["start"] and spans[1]["start"] >= spans[0]["start"]


def test_scan_reports_nothing_on_unmarked_audio(scan_value_setup):
    """20 s of unmarked audio (76 windows, 608 views): no span, and the largest confidence under the threshold."""
    plain, bits, y1, _ = scan_value_setup
    rng = np.random.default_rng(103)
    audio = (rng.standard_normal(320000) * np.sqrt(np.mean(y1[0].astype(np.float64) ** 2))).astype(F32)
    spans, prof = cpu_scan(plain, audio)
    print(f"unmarked: {len(prof['starts'])} windows, largest win_conf {prof['win_conf'].max():.4f}, "
          f"99th percentile {np.percentile(prof['win_conf'], 99):.4f}")
    assert spans == [] and prof["n_segments"] == 0
    assert float(prof["win_conf"].max()) < MIN_CONFIDENCE
