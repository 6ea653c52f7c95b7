"""Coded payloads (EXTENSION) on the CPU: the code and its Viterbi decoder as utils/watermark/fec.py states them (encoder,
free distance, maximum likelihood against brute force, hard errors, erasures, the CRC), the card key and the messages, the C
ABI's refusals, the kernel body compiled for the host (tests/host_sim/viterbi_check.cpp) against the restatement, and the
value claim on the CPU oracle.  DESIGN.md section 29."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, make_clip
from oracle import aware_oracle as O
from aware_amd.utils.watermark import fec

F32 = np.float32
RATE_OF = {2: "1/2", 3: "1/3"}


def bipolar(bits):
    return (2 * np.asarray(bits, dtype=np.int64) - 1).astype(F32)


# ---- 1. the code ------------------------------------------------------------------------------------------------------------------
def plain_encode(bits, polys):
    """The issue's encoder, bit by bit."""
    s, out = 0, []
    for b in bits:
        r = (int(b) << 6) | s
        out += [bin(r & p).count("1") & 1 for p in polys]
        s = r >> 1
    return out


@pytest.mark.parametrize("rate,polys", [("1/2", (0o171, 0o133)), ("1/3", (0o133, 0o171, 0o165))])
def test_encoder_against_a_plain_loop(rate, polys):
    rng = np.random.default_rng(1)
    assert fec.RATES[rate] == polys
    for T in (1, 7, 40, 256):
        bits = rng.integers(0, 2, (5, T))
        got = fec.conv_encode(bits, rate)
        assert got.shape == (5, len(polys) * T) and got.dtype == np.int32
        for r in range(5):
            assert got[r].tolist() == plain_encode(bits[r], polys)
    # the impulse response reads the generators out, MSB first: 0o171 = 1111001, 0o133 = 1011011, interleaved
    assert fec.conv_encode(np.array([1, 0, 0, 0, 0, 0, 0]), "1/2").tolist() == [1, 1, 1, 0, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1]


@pytest.mark.parametrize("rate,dfree", [("1/2", 10), ("1/3", 15)])
def test_minimum_distance(rate, dfree):
    """The smallest weight of a non-zero terminated codeword over all messages of up to 10 bits: the known free distances
    of these generators, which pins the polynomials and the bit order."""
    msgs = (np.arange(1, 1024)[:, None] >> np.arange(10)) & 1
    words = fec.conv_encode(np.concatenate([msgs, np.zeros((1023, fec.TAIL), dtype=np.int64)], axis=1), rate)
    assert int(words.sum(axis=1).min()) == dfree


def test_crc_hand_values():
    """CRC-8 (0x07) and CRC-16 (0x1021, the CCITT-FALSE check value) of "123456789", register all ones, MSB first."""
    bits = np.unpackbits(np.frombuffer(b"123456789", dtype=np.uint8))
    assert int(fec.crc_register(bits, 16)) == 0x29B1
    assert int(fec.crc_register(bits, 8)) == 0xFB
    assert fec.crc_bits(bits, 16).tolist() == [int(b) for b in f"{0x29B1:016b}"]
    assert fec.crc_bits(bits, 0).shape == (0,)


@pytest.mark.parametrize("rate,L,c", [("1/2", 64, 8), ("1/2", 65, 8), ("1/3", 64, 0), ("1/3", 128, 8), ("1/2", 512, 16)])
def test_frame_layout_and_clean_round_trip(rate, L, c):
    n = len(fec.RATES[rate])
    T = L // n
    k = fec.capacity(L, rate, c)
    assert k == T - 6 - c
    msg = np.random.default_rng(L + c).integers(0, 2, k)
    frame = fec.encode_frame(msg, L, rate, c)
    assert frame.shape == (L,) and set(np.unique(frame)) <= {0, 1} and not frame[n * T:].any()
    inputs = np.concatenate([msg, fec.crc_bits(msg, c), np.zeros(6, dtype=np.int64)])
    assert frame[:n * T].tolist() == plain_encode(inputs, fec.RATES[rate])
    out = fec.viterbi_decode(bipolar(frame)[None], 0.0, rate, c)
    assert out["bits"].shape == (1, T) and out["bits"][0].tolist() == inputs.tolist()
    assert out["valid"][0] and out["corrected"][0] == 0 and out["metric"][0] == F32(n * T)
    assert out["metric"].dtype == F32 and out["corrected"].dtype == np.int32 and out["valid"].dtype == bool


# ---- 2. the decoder -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", ["1/2", "1/3"])
@pytest.mark.parametrize("c,k", [(0, 10), (8, 2), (8, 10)])
def test_decoder_against_brute_force(rate, c, k):
    """Maximum correlation over every frame.  The decoder maximises over all 2^(k + c) input sequences, CRC-valid or not: with
    c = 8 and k = 2 that whole set is enumerated and all decoded bits are compared; over the 2^k frames of a message the
    decoded message is compared wherever the decode is valid (then the best sequence is a frame) or c = 0.  Rows whose best
    two correlations are closer than 1e-3 are left out: the maximum has to be unique."""
    n = len(fec.RATES[rate])
    T = k + c + 6
    L = n * T + 1
    rng = np.random.default_rng(100 * c + k + n)
    free = k + c if k + c <= 10 else k                      # the bits that are enumerated
    seqs = (np.arange(1 << free)[:, None] >> np.arange(free)) & 1
    if free == k and c:
        seqs = np.concatenate([seqs, fec.crc_bits(seqs, c)], axis=1)
    words = bipolar(fec.conv_encode(np.concatenate([seqs, np.zeros((len(seqs), 6), dtype=np.int64)], axis=1), rate)).astype(np.float64)
    sent = rng.integers(0, 2, (96, k))
    frames = np.stack([fec.encode_frame(m, L, rate, c) for m in sent])
    sigma = np.repeat([0.5, 1.0, 1.6], 32)[:, None]
    values = (bipolar(frames) + sigma * rng.standard_normal(frames.shape)).astype(F32)
    out = fec.viterbi_decode(values, 0.0, rate, c)
    corr = values[:, :n * T].astype(np.float64) @ words.T    # [rows, sequences]
    order = np.sort(corr, axis=1)
    unique = order[:, -1] - order[:, -2] > 1e-3
    best = seqs[np.argmax(corr, axis=1)]
    rows = unique & (out["valid"] if free == k and c else True)
    assert rows.sum() >= 24, rows.sum()
    width = k if free == k else k + c
    assert np.array_equal(out["bits"][rows, :width], best[rows, :width])
    if c == 0 or free == k + c:                             # the enumeration is the decoder's whole search space
        np.testing.assert_allclose(out["metric"][unique], order[unique, -1], rtol=1e-5, atol=1e-4)
    assert (out["bits"][:, k + c:] == 0).all()             # the tail always decodes to zeros: the traceback ends in state 0
    assert 0 < np.count_nonzero(out["bits"][:, :k] != sent) < sent.size     # the noise is strong enough to matter


@pytest.mark.parametrize("rate,flips,L,c", [("1/2", 4, 64, 8), ("1/3", 7, 96, 8), ("1/2", 4, 512, 16), ("1/3", 7, 128, 0)])
def test_hard_errors_within_half_the_free_distance(rate, flips, L, c):
    """With +-1 inputs any 4 flipped positions at rate 1/2 and any 7 at rate 1/3 decode to the sent message: 200 seeded
    patterns each."""
    n = len(fec.RATES[rate])
    T = L // n
    k = fec.capacity(L, rate, c)
    rng = np.random.default_rng(7 * L + flips)
    sent = rng.integers(0, 2, (200, k))
    values = bipolar(np.stack([fec.encode_frame(m, L, rate, c) for m in sent]))
    for r in range(200):
        at = rng.choice(n * T, size=flips, replace=False) if r % 2 else rng.integers(0, n * T - flips) + np.arange(flips)
        values[r, at] *= -1                                  # scattered patterns and bursts
    out = fec.viterbi_decode(values, 0.0, rate, c)
    assert np.array_equal(out["bits"][:, :k], sent)
    assert out["valid"].all() and (out["corrected"] == flips).all()
    assert (out["metric"] == F32(n * T - 2 * flips)).all()


def test_erasures():
    """NaN and inf positions count as 0 and the row still decodes; a row of nothing else decodes to the all-zero path."""
    rng = np.random.default_rng(3)
    k = fec.capacity(128, "1/3", 8)
    sent = rng.integers(0, 2, (6, k))
    frames = np.stack([fec.encode_frame(m, 128, "1/3", 8) for m in sent])
    values = (bipolar(frames) + 0.3 * rng.standard_normal(frames.shape)).astype(F32)
    clean = values.copy()
    for r, bad in enumerate((np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf)):
        values[r, rng.choice(126, size=12, replace=False)] = bad
    out = fec.viterbi_decode(values, 0.0, "1/3", 8)
    assert np.array_equal(out["bits"][:, :k], sent) and out["valid"].all() and np.isfinite(out["metric"]).all()
    zeroed = np.where(np.isfinite(values), clean, 0).astype(F32)
    same = fec.viterbi_decode(zeroed, 0.0, "1/3", 8)
    for key in ("bits", "metric", "valid", "corrected"):
        assert np.array_equal(out[key], same[key]), key
    # inf - centre and (-inf) - centre stay erasures with a centre, and a value that overflows in v - centre is one too
    shifted = fec.viterbi_decode(values + F32(0.5), 0.5, "1/3", 8)
    assert np.array_equal(shifted["bits"][:, :k], sent)
    assert fec.soft_values(np.array([3e38, -3e38, 1.0], dtype=F32), -3e38).tolist() == [0.0, 0.0, float(F32(3e38))]
    gone = fec.viterbi_decode(np.full((1, 128), np.nan, dtype=F32), 0.0, "1/3", 8)
    assert not gone["bits"].any() and gone["metric"][0] == 0 and gone["corrected"][0] == 0 and not gone["valid"][0]


def test_crc_refuses_the_all_zero_frame():
    for c in (8, 16):
        for rate in ("1/2", "1/3"):
            out = fec.viterbi_decode(np.zeros((1, 256), dtype=F32), 0.0, rate, c)
            assert not out["bits"].any() and out["metric"][0] == 0 and not out["valid"][0]
            # the all-zero INPUT sequence sent on purpose (all coded bits 0) is refused as well
            out = fec.viterbi_decode(np.full((1, 256), -1, dtype=F32), 0.0, rate, c)
            assert not out["bits"].any() and out["corrected"][0] == 0 and not out["valid"][0]
    assert fec.viterbi_decode(np.zeros((1, 256), dtype=F32), 0.0, "1/2", 0)["valid"][0]      # c = 0: a finite metric
    big = np.full((1, 64), 3e38, dtype=F32)
    assert not fec.viterbi_decode(big, 0.0, "1/2", 0)["valid"][0]                                # the metric overflows


def test_crc16_false_accepts_on_pure_noise():
    """4096 rows of Gaussian soft values at L = 512, rate 1/2, CRC-16: the expected count of valid rows is 4096 / 65536 =
    0.06; at most 2 (the chance of more is 4e-5).  Measured: DESIGN.md section 29."""
    values = np.random.default_rng(2024).standard_normal((4096, 512)).astype(F32)
    out = fec.viterbi_decode(values, 0.0, "1/2", 16)
    count = int(out["valid"].sum())
    print(f"CRC-16 on pure noise: {count} of 4096 rows valid; corrected {out['corrected'].mean():.1f} of 512 on average")
    assert count <= 2


# ---- 3. the card key, the messages, the C ABI -------------------------------------------------------------------------------------------
def test_capacity_and_parser():
    assert fec.capacity(64, "1/2", 8) == 18 and fec.capacity(128, "1/3", 8) == 28 and fec.capacity(128, "1/2", 16) == 42
    assert fec.capacity(14, "1/2", 0) == 1 and fec.capacity(512, "1/3", 0) == 164 and fec.capacity(20, "1/2", 0) == 4
    for L, rate, c in ((13, "1/2", 0), (20, "1/3", 0), (20, "1/2", 8), (64, "1/3", 16), (29, "1/2", 8)):
        with pytest.raises(ValueError) as e:
            fec.capacity(L, rate, c)
        assert str(L) in str(e.value) and rate in str(e.value) and f"{c} bits" in str(e.value)
    assert fec.check_payload_code(None) is None
    assert fec.check_payload_code({"rate": "1/2", "crc": 16}) == {"rate": "1/2", "crc": 16}
    assert fec.check_payload_code({"rate": "1/3"}) == {"rate": "1/3", "crc": 0}
    for bad, word in (({"rate": "1/4"}, "rate"), ({"rate": 0.5}, "rate"), ({"crc": 8}, "rate"), ({"rate": "1/2", "crc": 4}, "crc"),
                      ({"rate": "1/2", "crc": "8"}, "crc"), ({"rate": "1/2", "crc": True}, "crc"), ({"rate": "1/2", "crc": 8.0}, "crc"),
                      ({"rate": "1/2", "k": 7}, "'k'"), ("1/2", "mapping"), (3, "mapping"), ([("rate", "1/2")], "mapping")):
        with pytest.raises(ValueError, match=word):
            fec.check_payload_code(bad)


def test_messages():
    k = 18
    bits = np.random.default_rng(4).integers(0, 2, k)
    assert fec.message_bits(bits, k).tolist() == bits.tolist() and fec.message_bits(bits.tolist(), k).dtype == np.int32
    assert fec.message_bits(b"\xa5\x01", k).tolist() == [1, 0, 1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0]
    assert fec.message_bits(b"\xff", k).tolist() == [1] * 8 + [0] * 10 and fec.message_bits(b"", k).tolist() == [0] * k
    assert fec.message_bytes(fec.message_bits(b"\xa5\x01", k)) == b"\xa5\x01" and fec.message_bytes(np.ones(7)) == b""
    for bad in (bits[:-1], np.concatenate([bits, [0]]), b"\x00\x00\x00", bits.reshape(2, 9), np.full(k, 2), np.full(k, 0.5)):
        with pytest.raises(ValueError):
            fec.message_bits(bad, k)
    with pytest.raises(ValueError):
        fec.encode_frame(bits, 64, "1/2", 16)               # k = 10 there
    with pytest.raises(ValueError):
        fec.viterbi_decode(np.zeros(64, dtype=F32), 0.0, "1/2", 8)


def test_card_key_reaches_embedder_and_detector(tmp_path):
    from aware_amd import service
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        text = f.read()
    assert '# payload_code: {rate: "1/2", crc: 16}' in text
    card = yaml.safe_load(text)
    assert "payload_code" not in card                          # the committed card keeps its keys
    emb, det = load()
    assert emb.payload_code is None and det.payload_code is None
    with pytest.raises(ValueError, match="payload_code"):
        service.embed_message(np.zeros(16000, dtype=F32), 16000, b"\x01", emb)
    with pytest.raises(ValueError, match="payload_code"):
        service.detect_message(np.zeros(16000, dtype=F32), 16000, det)
    with pytest.raises(ValueError, match="payload_code"):
        service.detect_message_batch([np.zeros(16000, dtype=F32)], 16000, det)
    with pytest.raises(ValueError, match="payload_code"):
        det.decode_messages(np.zeros((1, 20), dtype=F32))
    p = tmp_path / "card.yaml"
    card["detection_net_cfg"] = dict(card["detection_net_cfg"], output_length=64)
    card["watermark_length"] = 64
    card["payload_code"] = {"rate": "1/2", "crc": 8}
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.payload_code == {"rate": "1/2", "crc": 8} == det.payload_code
    with pytest.raises(ValueError, match="18 bits"):           # a message of the wrong length, before anything runs
        service.embed_message(np.zeros(16000, dtype=F32), 16000, np.zeros(17, dtype=int), emb)
    with pytest.raises(ValueError, match="18 bits"):
        service.embed_message_batch([np.zeros(16000, dtype=F32)], 16000, [b"\x00\x00\x00"], emb)
    with pytest.raises(ValueError, match="sample rate"):
        service.embed_message(np.zeros(16000, dtype=F32), 8000, b"\x01", emb)
    with pytest.raises(ValueError, match="sample rate"):
        service.detect_message(np.zeros(16000, dtype=F32), 8000, det)
    card["payload_code"] = {"rate": "1/3"}
    p.write_text(yaml.safe_dump(card))
    assert load(str(p))[1].payload_code == {"rate": "1/3", "crc": 0}
    for bad in ({"rate": "1/4"}, {"rate": "1/2", "crc": 12}, {"crc": 8}, {"rate": "1/2", "bits": 8}, "1/2", 2,
                {"rate": "1/3", "crc": 16}):                   # the last: 64 // 3 - 6 - 16 < 1
        card["payload_code"] = bad
        p.write_text(yaml.safe_dump(card))
        assert load(str(p)) is None, bad


def test_abi_symbol_and_bad_arguments():
    from aware_amd import _lib, runtime as rt, service
    lib = _lib.load_library()
    assert "aware_viterbi_decode" in _lib.SIGNATURES and hasattr(lib, "aware_viterbi_decode")
    assert len(_lib.SIGNATURES["aware_viterbi_decode"][1]) == 11 and "viterbi_kernels.hip" in _lib.SOURCES
    assert lib.aware_version() == 350
    with open(os.path.join(ROOT, "include", "aware_hip.h")) as f:
        assert "int aware_viterbi_decode(const float* values, int R, int L, float centre, int rate_n, int crc_bits" in f.read()
    assert callable(rt.viterbi_decode)
    for name in ("embed_message", "embed_message_batch", "detect_message", "detect_message_batch"):
        assert callable(getattr(service, name)) and name in service.__all__
    p, q = C.c_void_p(256), C.c_void_p(512)                    # never dereferenced: every call below is refused

    def decode(values=p, R=4, L=64, centre=0.0, n=2, c=8, bits=q, metric=q, valid=q, corrected=q):
        return lib.aware_viterbi_decode(values, R, L, centre, n, c, bits, metric, valid, corrected, None)

    for kw in ({"values": None}, {"bits": None}, {"metric": None}, {"valid": None}, {"corrected": None}):
        assert decode(**kw) == -1, kw
    for kw in ({"R": 0}, {"R": -1}, {"R": (1 << 20) + 1}, {"L": 0}, {"L": -4}, {"L": 513}, {"n": 1}, {"n": 4}, {"n": 0},
               {"c": 4}, {"c": -8}, {"c": 32}, {"centre": float("nan")}, {"centre": float("inf")}, {"centre": float("-inf")},
               {"L": 29}, {"L": 13, "c": 0}, {"L": 20, "n": 3, "c": 0}, {"L": 64, "n": 3, "c": 16}, {"L": 45, "c": 16}):
        assert decode(**kw) == -1, kw


# ---- 4. the kernel body on the host ---------------------------------------------------------------------------------------------------
CASES = [(2, 14, 0), (2, 64, 8), (2, 65, 8), (3, 64, 0), (3, 128, 8), (2, 512, 16), (3, 512, 0)]
ROWS = (1, 3, 4, 5, 257)
CENTRES = {1: 0.0, 3: 0.5, 4: 0.0, 5: -0.25, 257: 0.5}


def decoder_case(n, L, c, R):
    """(values [R, L] float32, centre) of the kernel tests, also the device's.  Row r is of kind (r + R) % 8: 0 an exact +-1
    frame; 1, 2, 3 a frame in Gaussian noise of sigma 0.4, 0.8, 1.3; 4 pure noise; 5 all zeros, where every step is a tie;
    6 a noisy frame with NaN, +inf and -inf in it; 7 a frame scaled to a detector's small outputs.  Every row is offset by
    the case's centre, which is not zero for R = 3, 5 and 257.  The ignored positions beyond n T hold noise."""
    rate, centre = RATE_OF[n], CENTRES[R]
    rng = np.random.default_rng(1000 * L + 10 * c + R)
    k = fec.capacity(L, rate, c)
    y = np.zeros((R, L), dtype=np.float64)
    for r in range(R):
        kind = (r + R) % 8
        frame = bipolar(fec.encode_frame(rng.integers(0, 2, k), L, rate, c)).astype(np.float64)
        noise = rng.standard_normal(L)
        if kind == 0:
            y[r] = frame
        elif kind in (1, 2, 3):
            y[r] = frame + (0.4, 0.8, 1.3)[kind - 1] * noise
        elif kind == 4:
            y[r] = noise
        elif kind == 6:
            y[r] = frame + 0.5 * noise
            y[r, rng.choice(L, size=min(9, L // 2), replace=False)] = np.resize([np.nan, np.inf, -np.inf], min(9, L // 2))
        elif kind == 7:
            y[r] = 0.07 * frame + 0.05 * noise
        if kind not in (5, 6):
            y[r, n * (L // n):] = noise[n * (L // n):]
    return (y + centre).astype(F32), centre


def test_decoder_case_kinds():
    values, centre = decoder_case(2, 64, 8, 257)
    assert centre == 0.5 and (values[(5 - 257) % 8] == F32(0.5)).all() and np.isnan(values[(6 - 257) % 8]).any()
    assert np.isposinf(values).any() and np.isneginf(values).any()
    out = fec.viterbi_decode(values, centre, "1/2", 8)
    assert 60 < out["valid"].sum() < 257 and out["corrected"].max() > 10
    assert decoder_case(2, 14, 0, 1)[0].shape == (1, 14)


@pytest.fixture(scope="module")
def viterbi_check(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "host_sim", "viterbi_check.cpp")
    exe = str(tmp_path_factory.mktemp("viterbi") / "viterbi_check")
    subprocess.run(["c++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, src], check=True)
    return exe


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("n,L,c", CASES)
def test_kernel_body_on_the_host(viterbi_check, tmp_path, n, L, c):
    """viterbi_body.hpp compiled for the host under AddressSanitizer and UBSan, on the device test's cases: no report, and
    every output equal to fec.viterbi_decode bit for bit; nothing is written beyond the rows."""
    T, words = L // n, (L // n + 31) // 32
    for R in ROWS:
        values, centre = decoder_case(n, L, c, R)
        src, dst = tmp_path / f"in{R}.bin", tmp_path / f"out{R}.bin"
        with open(src, "wb") as f:
            f.write(np.array([R, L, n, c], dtype=np.int32).tobytes() + np.array([centre], dtype=F32).tobytes() + values.tobytes())
        done = subprocess.run([viterbi_check, str(src), str(dst)], capture_output=True, text=True)
        assert done.returncode == 0 and not done.stderr, done.stderr
        raw = np.fromfile(dst, dtype=np.uint32)
        assert raw.size == R * words + 3 * R
        bits, metric, valid, corrected = np.split(raw, [R * words, R * words + R, R * words + 2 * R])
        ref = fec.viterbi_decode(values, centre, RATE_OF[n], c)
        assert np.array_equal(bits.reshape(R, words), fec.pack_bits(ref["bits"])), (R, "bits")
        assert same_bits(metric.view(F32), ref["metric"]), (R, "metric")
        assert np.array_equal(valid.view(np.int32), ref["valid"].astype(np.int32)), (R, "valid")
        assert np.array_equal(corrected.view(np.int32), ref["corrected"]), (R, "corrected")


# ---- 5. the value claim, on the CPU oracle ---------------------------------------------------------------------------------------------
CLAIM = {"L": 64, "rate": "1/2", "crc": 8, "snr_db": 10.0}


def claim_messages(n_clips):
    return np.random.default_rng(5).integers(0, 2, (n_clips, fec.capacity(CLAIM["L"], CLAIM["rate"], CLAIM["crc"])))


def claim_figures(sent, frames, clean, noisy, reads_per_clip):
    """The value claim's figures and assertions, for the oracle here and the device in tests/test_gpu_coded_payload.py.
    sent [B, k], frames [B, L] bits, clean: decode dicts of the B clean reads, noisy: of the B * reads_per_clip noisy reads
    (clip-major), every dict with `values`."""
    k = sent.shape[1]
    for b, m in enumerate(clean):
        assert m["valid"] and np.array_equal(m["message"], sent[b]) and m["corrected"] == 0, b
        assert np.array_equal(m["values"] > 0, frames[b] > 0), b
    raw_wrong = np.array([np.count_nonzero((m["values"] > 0) != (frames[i // reads_per_clip] > 0)) for i, m in enumerate(noisy)])
    right = np.array([np.array_equal(m["message"], sent[i // reads_per_clip]) for i, m in enumerate(noisy)])
    valid = np.array([bool(m["valid"]) for m in noisy])
    reads = len(noisy)
    raw_ber = 100.0 * raw_wrong.sum() / (reads * frames.shape[1])
    whole = np.count_nonzero(raw_wrong == 0)
    coded = np.count_nonzero(right & valid)
    false_accepts = np.count_nonzero(~right & valid)
    print(f"coded payload, L = {frames.shape[1]}, rate {CLAIM['rate']}, CRC-{CLAIM['crc']}, k = {k}, noise {CLAIM['snr_db']} dB, "
          f"{reads} reads: raw BER {raw_ber:.2f} %, all raw bits right {whole} ({100.0 * whole / reads:.1f} %), coded message "
          f"right and valid {coded} ({100.0 * coded / reads:.1f} %), wrong and valid {false_accepts}")
    assert raw_ber >= 3.0
    assert whole <= 0.25 * reads
    assert coded >= 0.9 * reads
    assert false_accepts <= reads / 48.0
    return raw_ber, whole, coded, false_accepts


def test_coded_messages_survive_noise_that_breaks_raw_payloads():
    """output_length = 64, eight 1 s clips (seeds 0..7), plain 400-step embedding of rate-1/2 CRC-8 frames of 18-bit messages,
    then Gaussian noise at 10 dB, six seeds per clip: 48 reads.  Measured with this restatement: DESIGN.md section 29."""
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    plain = O.Embedder()
    ws, bs = O.detector_weights(output_length=CLAIM["L"])
    plain.det.ws, plain.det.bs = ws, bs
    sent = claim_messages(8)
    frames = np.stack([fec.encode_frame(m, CLAIM["L"], CLAIM["rate"], CLAIM["crc"]) for m in sent])
    marked = plain.embed(np.stack([make_clip(b, 16000)[0] for b in range(8)]), bipolar(frames))[0].numpy()

    def read(audio):
        values = plain.detect_raw(audio).numpy()
        out = fec.viterbi_decode(values, 0.0, CLAIM["rate"], CLAIM["crc"])
        return [{"message": out["bits"][r, :sent.shape[1]], "valid": out["valid"][r], "corrected": out["corrected"][r],
                 "values": values[r]} for r in range(len(values))]

    noisy = np.stack([O.gaussian_noise_attack(marked[b], CLAIM["snr_db"], seed=1000 * sd + b) for b in range(8) for sd in range(6)])
    claim_figures(sent, frames, read(marked), read(noisy), 6)
