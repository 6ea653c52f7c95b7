"""Coded payloads (EXTENSION) on the device: the Viterbi kernel of csrc/viterbi_kernels.hip
(aware_viterbi_decode) against the numpy restatement of utils/watermark/fec.py, bit for bit; messages embedded and read back
through the service calls under noise; and a coded clip found and decoded by the scan.

Run on the MI355X box:  python -m pytest tests/test_gpu_coded_payload.py -m gpu -q -s"""
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, make_clip
from test_coded_payload_host import CASES, CLAIM, RATE_OF, ROWS, claim_figures, claim_messages, decoder_case, same_bits
from test_scan_host import AT, splice

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from aware_amd import runtime
    from aware_amd._lib import require_gpu
    require_gpu()
    return runtime


@pytest.fixture(scope="module")
def fec():
    from aware_amd.utils.watermark import fec
    return fec


# ---- 1. the kernel alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,L,c", CASES)
def test_viterbi_kernel_matches_the_restatement(rt, fec, n, L, c):
    """Every output bit for bit, for 1, 3, 4, 5 and 257 rows (workgroups of four rows: a lone row, a group that is not full,
    a full one, one row over, many groups): exact frames, frames in noise at three levels, pure noise, all zeros (every step a
    tie), NaN and +-inf, small amplitudes; a centre that is not zero for three of the row counts."""
    T = L // n
    for R in ROWS:
        values, centre = decoder_case(n, L, c, R)
        ref = fec.viterbi_decode(values, centre, RATE_OF[n], c)
        out = {k: v.cpu().numpy() for k, v in rt.viterbi_decode(torch.from_numpy(values).cuda(), centre, RATE_OF[n], c).items()}
        assert out["bits"].shape == (R, (T + 31) // 32)
        assert np.array_equal(out["bits"].view(np.uint32), fec.pack_bits(ref["bits"])), (R, "bits")
        assert np.array_equal(fec.unpack_bits(out["bits"], T), ref["bits"])
        assert same_bits(out["metric"], ref["metric"]), (R, "metric")
        assert out["valid"].dtype == bool and np.array_equal(out["valid"], ref["valid"]), (R, "valid")
        assert np.array_equal(out["corrected"], ref["corrected"]), (R, "corrected")


def test_viterbi_wrapper_refuses_bad_arguments(rt):
    v = torch.zeros((4, 64), device="cuda")
    for args in ((v[0], 0.0, "1/2", 8), (v, 0.0, "1/4", 8), (v, 0.0, "1/2", 4), (v, float("nan"), "1/2", 8),
                 (v[:, :29], 0.0, "1/2", 8), (torch.zeros((1, 513), device="cuda"), 0.0, "1/2", 8), (v[:0], 0.0, "1/2", 8)):
        with pytest.raises(ValueError):
            rt.viterbi_decode(*args)


# ---- 2. end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def coded(rt, tmp_path_factory):
    """The card with 64 outputs and payload_code {rate 1/2, crc 8}; four 1 s clips (seeds 0..3) marked by embed_message_batch
    with the host claim's messages."""
    from aware_amd import service
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        card = yaml.safe_load(f)
    card["detection_net_cfg"] = dict(card["detection_net_cfg"], output_length=CLAIM["L"])
    card["watermark_length"] = CLAIM["L"]
    card["payload_code"] = {"rate": CLAIM["rate"], "crc": CLAIM["crc"]}
    p = tmp_path_factory.mktemp("coded") / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    sent = claim_messages(4)
    clips = [make_clip(b, 16000)[0] for b in range(4)]
    marked = service.embed_message_batch(clips, 16000, list(sent), emb)
    return emb, det, sent, clips, marked


def test_messages_survive_noise_end_to_end(coded, fec):
    """embed_message_batch, Gaussian noise at 10 dB (six seeds per clip, 24 reads), detect_message_batch: the host claim's
    bars.  The device's figures: DESIGN.md section 29."""
    from oracle import aware_oracle as O
    from aware_amd import service
    emb, det, sent, clips, marked = coded
    frames = np.stack([fec.encode_frame(m, CLAIM["L"], CLAIM["rate"], CLAIM["crc"]) for m in sent])
    clean = service.detect_message_batch(marked, 16000, det)
    noisy = service.detect_message_batch([O.gaussian_noise_attack(marked[b], CLAIM["snr_db"], seed=1000 * sd + b)
                                          for b in range(4) for sd in range(6)], 16000, det)
    claim_figures(sent, frames, clean, noisy, 6)
    # what a result holds, and that the decode is the restatement's on the detector's own values
    m = noisy[0]
    assert set(m) == {"message", "bytes", "valid", "corrected", "metric", "values"}
    assert m["message"].shape == (18,) and m["bytes"] == np.packbits(m["message"][:16].astype(np.uint8)).tobytes()
    ref = fec.viterbi_decode(np.stack([r["values"] for r in noisy]), 0.0, CLAIM["rate"], CLAIM["crc"])
    for r, got in enumerate(noisy):
        assert np.array_equal(got["message"], ref["bits"][r, :18]) and got["valid"] == ref["valid"][r]
        assert got["corrected"] == ref["corrected"][r] and np.float32(got["metric"]) == ref["metric"][r]


def test_single_clip_stereo_and_bytes(coded):
    from aware_amd import service
    emb, det, sent, clips, marked = coded
    one = service.detect_message(marked[1], 16000, det)
    assert one["valid"] and np.array_equal(one["message"], sent[1])
    unmarked = np.random.default_rng(9).standard_normal(len(marked[2])).astype(np.float32) * 0.1     # a marked clip is 15 872 samples
    for pair, want in (((marked[2], unmarked), 2), ((unmarked, marked[3]), 3)):
        got = service.detect_message(np.column_stack(pair), 16000, det)
        assert got["valid"] and np.array_equal(got["message"], sent[want])
    both = service.detect_message(np.column_stack([marked[0], marked[1]]), 16000, det)      # two valid ones: the larger metric
    l, r = (service.detect_message(marked[i], 16000, det) for i in (0, 1))
    assert both["valid"] and np.array_equal(both["message"], (r if r["metric"] > l["metric"] else l)["message"])
    # bytes in, bytes out; embed_message on a stereo clip marks both channels
    stereo = service.embed_message(np.column_stack([clips[0], clips[1]]), 16000, b"\xc3\x5a", emb)
    assert stereo.shape == (len(marked[0]), 2)
    for ch in (0, 1):
        got = service.detect_message(stereo[:, ch], 16000, det)
        assert got["valid"] and got["bytes"] == b"\xc3\x5a" and got["message"][16:].tolist() == [0, 0]
    # the uncoded calls read the same clip as before: the frame's own bits
    assert service.detect_watermark(marked[1], 16000, det).shape == (64,)


# ---- 3. the scan --------------------------------------------------------------------------------------------------------------------------
def test_scan_decodes_the_span(coded):
    """A coded 1 s clip inside 9 s of unmarked audio: one span, valid, with the message; the same scan by a detector without
    the code returns the same spans without the three keys."""
    from aware_amd import service
    emb, det, sent, clips, marked = coded
    audio = splice(marked[0], 144000, 100)
    spans = det.scan([audio], 16000)[0]
    assert len(spans) == 1
    s = spans[0]
    print(f"coded span {s['start']}..{s['end']} peak {s['peak']} confidence {s['confidence']:.4f} valid {s['valid']} "
          f"corrected {s['corrected']}")
    assert s["valid"] and np.array_equal(s["message"], sent[0]) and abs(s["peak"] - AT) <= 64
    found = service.scan_watermark(audio, 16000, det)
    assert len(found) == 1 and found[0]["valid"] and np.array_equal(found[0]["message"], sent[0])
    assert found[0]["corrected"] == s["corrected"] and found[0]["payload"].shape == (64,)
    code, det.payload_code = det.payload_code, None
    try:
        plain = det.scan([audio], 16000)[0]
        served = service.scan_watermark(audio, 16000, det)
    finally:
        det.payload_code = code
    assert len(plain) == 1 and set(plain[0]) == {"start", "end", "peak", "confidence", "values", "windows"}
    assert set(served[0]) == {"start", "end", "peak", "confidence", "payload", "values"}
    for key in ("start", "end", "peak", "confidence", "windows"):
        assert plain[0][key] == s[key], key
    assert np.array_equal(plain[0]["values"], s["values"])
    assert det.scan([audio], 16000, min_confidence=0.9) == [[]]            # no span: nothing to decode, no launch
