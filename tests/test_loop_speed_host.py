"""Speed change inside the embed loop (EXTENSION): the torch restatement (aware_amd/embedding/loop_attacks.py: speed_range,
speed_offset, speed_change, apply_chain) against a plain numpy loop of its definition, the gather-form adjoint against autograd,
the validation of the entry, the card keys, the C ABI's symbols, and the value claim on the CPU -- what a speed change inside
the loop buys against an independent polyphase resampler, through the oracle's embed loop.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, make_clip
from oracle import aware_oracle as O
from aware_amd.embedding import loop_attacks as LA
from test_loop_attacks_host import AttackedEmbedder, ber, unit_clip

SPEED = {"kind": "speed_change", "cents": 200.0}
NOISE10 = {"kind": "gaussian_noise", "snr_db": 10.0}
SUP = {"kind": "sample_suppression", "seconds": 0.3}
REVERB = {"kind": "reverberation", "rt60": 0.3}
M_MIN, M_MAX = -13520, 17034                               # ceil / floor of 65536 (2^(-+400 / 1200) - 1)


def weights(f):
    return (((-f + 2) * f - 1) * f / 2, ((3 * f - 5) * f * f + 2) / 2, ((-3 * f + 4) * f + 1) * f / 2, (f - 1) * f * f / 2)


def speed_loop(x, m, n_out):
    """The definition, sample by sample, in float64 and Python integers."""
    n, R = len(x), 65536 + m
    z = np.zeros(n_out)
    for i in range(n_out):
        p = i * R
        if p > (n - 1) << 16:
            continue
        i0, f = p >> 16, (p & 0xFFFF) / 65536.0
        acc = None
        for t, w in zip((-1, 0, 1, 2), weights(f)):
            term = w * (x[i0 + t] if 0 <= i0 + t < n else 0.0)
            acc = term if acc is None else acc + term
        z[i] = acc
    return z


def speed_adjoint_gather(gy, m, n):
    """gx[j] = sum over ascending i of w_{j - i0(i)}(f_i) gy[i], i in [ceil(((j - 2) << 16) / R), floor((((j + 2) << 16) - 1) / R)]
    and [0, n_out), j - i0(i) in -1..2, p_i <= (n - 1) << 16: the form the device kernel takes, no scatter."""
    R, n_out = 65536 + m, len(gy)
    gx = np.zeros(n)
    most = 0
    for j in range(n):
        lo = max(0, -((-((j - 2) << 16)) // R))
        hi = min(n_out - 1, (((j + 2) << 16) - 1) // R)
        most = max(most, hi - lo + 1)
        for i in range(lo, hi + 1):
            p = i * R
            t = j - (p >> 16)
            if -1 <= t <= 2 and p <= (n - 1) << 16:
                gx[j] += weights((p & 0xFFFF) / 65536.0)[t + 1] * gy[i]
    return gx, most


# ---- 1. the restatement -------------------------------------------------------------------------------------------------------
def test_speed_range_of_the_widest_entry():
    e = LA.parse_chain([{"kind": "speed_change", "cents": 400.0}])[0]
    assert e["cents"] == [-400.0, 400.0] and LA.speed_range(e) == (M_MIN, M_MAX)
    assert LA.speed_range(LA.parse_chain([SPEED])[0]) == (-7150, 8025)
    assert LA.speed_range(LA.parse_chain([{"kind": "speed_change", "cents": [0.0, 0.0]}])[0]) == (0, 0)
    # the range of offsets lies inside the range of cents
    for lo, hi in ((-400.0, 400.0), (-17.0, 84.0), (3.0, 165.0)):
        m_lo, m_hi = LA.speed_range({"cents": [lo, hi]})
        assert 1200 * np.log2(1 + m_lo / 65536) >= lo > 1200 * np.log2(1 + (m_lo - 1) / 65536)
        assert 1200 * np.log2(1 + m_hi / 65536) <= hi < 1200 * np.log2(1 + (m_hi + 1) / 65536)


@pytest.mark.parametrize("n", [4099, 7937])
@pytest.mark.parametrize("m", [M_MIN, M_MAX, -1, 0, 1])
def test_speed_change_is_the_definition(n, m):
    """Exact in float64 against the sample-by-sample loop, with the clip's own length and with the true-speed length."""
    x = unit_clip(3, n)
    for n_out in (n, LA.speed_length(n, m)):
        z = LA.speed_change(x, m, n_out)
        assert z.dtype == torch.float64 and z.shape == (n_out,)
        np.testing.assert_array_equal(z.numpy(), speed_loop(x.numpy(), m, n_out))
    assert LA.speed_length(n, m) == ((n - 1) << 16) // (65536 + m) + 1
    if m == 0:
        assert LA.speed_change(x, 0) is x and LA.speed_length(n, 0) == n
    # a faster clip ends in zeros, a slower one is truncated; the last live sample is the one at or before (n - 1) << 16
    z = LA.speed_change(x, m).numpy()
    live = LA.speed_length(n, m)
    if m > 0:
        assert live < n and np.all(z[live:] == 0.0) and z[live - 1] != 0.0
    elif m < 0:
        assert live >= n and z[-1] != 0.0
    z32 = LA.speed_change(x.float(), m)
    assert z32.dtype == torch.float32 and float((z32.double() - torch.as_tensor(z)).abs().max()) < 1e-6
    # batched input: the operator acts on the last axis
    xb = torch.stack([x, -2 * x])
    np.testing.assert_array_equal(LA.speed_change(xb, m)[1].numpy(), -2 * z)


def test_speed_change_reproduces_quadratics():
    # Catmull-Rom reproduces quadratics away from the ends, so a parabola comes out at the stretched positions
    n, m = 4099, 3000
    t = np.arange(n, dtype=np.float64)
    z = LA.speed_change(torch.from_numpy(0.5 + 1e-3 * t + 1e-6 * t * t), m).numpy()
    pos = np.arange(n) * (65536 + m) / 65536.0
    live = LA.speed_length(n, m) - 2
    np.testing.assert_allclose(z[2:live], (0.5 + 1e-3 * pos + 1e-6 * pos * pos)[2:live], rtol=1e-12)


@pytest.mark.parametrize("m", [-7000, -1, 0, 3, 8000, M_MIN, M_MAX])
def test_gather_adjoint_is_autograd(m):
    """The adjoint the device kernel computes, written out in numpy, against autograd on the restatement: within 1e-14."""
    n = 1531
    for n_out in (n, LA.speed_length(n, m)):
        x = unit_clip(7, n).requires_grad_(True)
        gy = np.cos(0.37 * np.arange(n_out)) * np.linspace(0.2, 1.0, n_out)
        (LA.speed_change(x, m, n_out) * torch.from_numpy(gy)).sum().backward()
        gx, most = speed_adjoint_gather(gy, m, n)
        assert most <= 7
        err = float(np.abs(x.grad.numpy() - gx).max())
        assert err <= 1e-14, (m, n_out, err)


def test_offsets_cover_the_closed_range():
    m_lo, m_hi = -3, 4
    got = [LA.speed_offset(LA.entry_draw(5, s, 0)[3], m_lo, m_hi) for s in range(400)]
    assert set(got) == set(range(m_lo, m_hi + 1))
    assert LA.speed_offset(0, M_MIN, M_MAX) == M_MIN and LA.speed_offset(0xFFFFFFFF, M_MIN, M_MAX) == M_MAX
    assert LA.speed_offset(12345, 77, 77) == 77
    wide = [LA.speed_offset(LA.entry_draw(5, s, 0)[3], M_MIN, M_MAX) for s in range(400)]
    assert M_MIN <= min(wide) < M_MIN + 500 and M_MAX - 500 < max(wide) <= M_MAX      # 400 draws on 30555 values
    assert abs(np.mean(wide) - (M_MIN + M_MAX) / 2) < 3 * (M_MAX - M_MIN) / np.sqrt(12 * 400)     # uniform in the ratio


def test_draws_differ_between_steps_and_clips():
    e = LA.parse_chain([SPEED])[0]
    ms = {(sd, s): LA.speed_offset(LA.entry_draw(sd, s, 0)[3], *LA.speed_range(e)) for sd in range(4) for s in range(8)}
    assert len(set(ms.values())) >= 30                                                    # 32 draws on 15176 values
    x = torch.stack([unit_clip(1), unit_clip(1)])
    z0, z1 = LA.apply_chain(x, [SPEED], [0, 1], 0), LA.apply_chain(x, [SPEED], [0, 1], 1)
    assert float((z0[0] - z0[1]).abs().max()) > 0.1 and float((z0[0] - z1[0]).abs().max()) > 0.1
    np.testing.assert_array_equal(LA.apply_chain(x, [SPEED], [0, 1], 0).numpy(), z0.numpy())      # reproducible
    np.testing.assert_array_equal(z0[1].numpy(), LA.speed_change(x[1], ms[(1, 0)]).numpy())
    # the entry's index keys the draw, and lane 3 is its own: the suppression's start (lane 1) does not move with it
    shifted = LA.apply_chain(x[:1], [dict(NOISE10, prob=0.0), SPEED], [0], 0)[0]
    m1 = LA.speed_offset(LA.entry_draw(0, 0, 1)[3], *LA.speed_range(e))
    np.testing.assert_array_equal(shifted.numpy(), LA.speed_change(x[0], m1).numpy())


def test_probability_and_identity():
    x = unit_clip(4)[None]
    for step in range(5):
        np.testing.assert_array_equal(LA.apply_chain(x, [dict(SPEED, prob=0.0)], [9], step).numpy(), x.numpy())
    fired = sum(int(not torch.equal(LA.apply_chain(x[:, :512], [dict(SPEED, prob=0.75)], [2], s), x[:, :512])) for s in range(400))
    assert 0.68 * 400 < fired < 0.82 * 400, fired                                         # 0.75 +- 3 sigma of 400 draws


def test_order_with_noise_and_suppression():
    x = unit_clip(6)[None]
    e = LA.parse_chain([dict(SPEED, cents=[300.0, 400.0])])[0]                            # a fast clip: a long run of zeros at its end
    m = LA.speed_offset(LA.entry_draw(1, 0, 0)[3], *LA.speed_range(e))
    res = LA.apply_chain(x, [e], [1], 0)[0]
    np.testing.assert_array_equal(res.numpy(), LA.speed_change(x[0], m).numpy())
    # noise behind the speed change: its sigma comes from the resampled signal (the clip ends in zeros)
    both = LA.apply_chain(x, [e, NOISE10], [1], 0)[0]
    sigma = np.sqrt(float((res ** 2).mean()) / 10.0)
    np.testing.assert_allclose((both - res).numpy(), sigma * LA.normal_draws(16000, 1, 0, 1), atol=1e-12)
    # noise in front: it is resampled too (the offset is entry 1's)
    front = LA.apply_chain(x, [NOISE10, e], [1], 0)[0]
    noisy = LA.apply_chain(x, [NOISE10], [1], 0)[0]
    m1 = LA.speed_offset(LA.entry_draw(1, 0, 1)[3], *LA.speed_range(e))
    np.testing.assert_array_equal(front.numpy(), LA.speed_change(noisy, m1).numpy())
    # a suppression in front is resampled with the clip: the gap moves and shrinks; behind, it is where it was drawn
    a = LA.apply_chain(x, [SUP, e], [1], 0)[0]
    b = LA.apply_chain(x, [e, SUP], [1], 0)[0]
    s_b = LA.suppression_start(LA.entry_draw(1, 0, 1)[1], 16000, 4800)
    assert float(b[s_b:s_b + 4800].abs().max()) == 0.0
    s_a = LA.suppression_start(LA.entry_draw(1, 0, 0)[1], 16000, 4800)
    inner = slice(int((s_a + 2) * 65536 / (65536 + m1)) + 2, int((s_a + 4798) * 65536 / (65536 + m1)) - 2)
    assert float(a[inner].abs().max()) == 0.0 and inner.stop - inner.start < 4800 * 65536 / (65536 + m1)


def test_ragged_lists():
    clips = [unit_clip(1, 7937), unit_clip(2, 40000)]
    out = LA.apply_chain(clips, [SPEED], [4, 5], 2)
    assert isinstance(out, list) and [len(o) for o in out] == [7937, 40000]
    np.testing.assert_array_equal(out[1].numpy(), LA.apply_chain(clips[1][None], [SPEED], [5], 2)[0].numpy())


# ---- 2. validation, card keys, ABI ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [
    [{"kind": "speed"}],
    [{"kind": "speed_change"}],
    [{"kind": "speed_change", "prob": 0.5}],
    [{"kind": "speed_change", "cents": 0.0}],
    [{"kind": "speed_change", "cents": -50.0}],
    [{"kind": "speed_change", "cents": [50.0, -50.0]}],
    [{"kind": "speed_change", "cents": 400.5}],
    [{"kind": "speed_change", "cents": [-401.0, 0.0]}],
    [{"kind": "speed_change", "cents": [0.0, 1200.0]}],
    [{"kind": "speed_change", "cents": float("nan")}],
    [{"kind": "speed_change", "cents": [float("nan"), 10.0]}],
    [{"kind": "speed_change", "cents": [-10.0, float("inf")]}],
    [{"kind": "speed_change", "cents": [1.0, 2.0, 3.0]}],
    [{"kind": "speed_change", "cents": "fast"}],
    [{"kind": "speed_change", "cents": 200.0, "prob": 1.5}],
    [{"kind": "speed_change", "cents": 200.0, "rt60": 0.3}],
    [{"kind": "speed_change", "cents": 200.0, "snr_db": 10.0}],
    [{"kind": "speed_change", "cents": 200.0, "seconds": 0.3}],
    [{"kind": "speed_change", "cents": 200.0}, {"kind": "speed_change", "cents": 100.0}],
    [{"kind": "speed_change", "cents": 200.0}, NOISE10, {"kind": "speed_change", "cents": 100.0}],
    [{"kind": "speed_change", "cents": 200.0}, REVERB],
    [REVERB, NOISE10, {"kind": "speed_change", "cents": 200.0}],
    [{"kind": "speed_change", "cents": [1.0, 1.00001]}],                                  # no offset inside: m_lo = 38 > m_hi = 37
    [{"kind": "speed_change", "cents": [-0.02, -0.01]}],
    [{"kind": "speed_change", "cents": 200.0}, NOISE10, SUP, NOISE10, SUP],
])
def test_invalid_chains_are_refused(chain):
    with pytest.raises(ValueError):
        LA.parse_chain(chain)
    from aware_amd.embedding import AWAREEmbedder
    with pytest.raises(ValueError):
        AWAREEmbedder(loss="push_extremes", verbose=False, loop_attacks=chain)


def test_parse_fills_defaults():
    assert LA.KINDS["speed_change"] == 3 and LA.KINDS["reverberation"] == 2 and LA.MAX_CENTS == 400.0
    c = LA.parse_chain([{"kind": "sample_suppression", "seconds": 0.5}, {"kind": "speed_change", "cents": 200},
                        {"kind": "gaussian_noise", "snr_db": 10}])
    assert c == [{"kind": "sample_suppression", "prob": 1.0, "seconds": 0.5},
                 {"kind": "speed_change", "prob": 1.0, "cents": [-200.0, 200.0]},
                 {"kind": "gaussian_noise", "prob": 1.0, "snr_db": 10.0}]
    assert LA.parse_chain(c) == c                                                          # a parsed chain parses to itself
    assert LA.device_entries_ex(c, 16000) == [(1, 1.0, [8000.0, 0.0, 0.0, 0.0]), (3, 1.0, [-7150.0, 8025.0, 0.0, 0.0]),
                                              (0, 1.0, [10.0, 0.0, 0.0, 0.0])]
    r = LA.parse_chain([{"kind": "speed_change", "cents": (-17, 84), "prob": 0.75}])
    assert r == [{"kind": "speed_change", "prob": 0.75, "cents": [-17.0, 84.0]}]
    assert LA.device_entries_ex(r, 16000) == [(3, 0.75, [-640.0, 3258.0, 0.0, 0.0])]
    one = LA.parse_chain([{"kind": "speed_change", "cents": [0.0, 0.0]}])                  # one value: the identity
    assert LA.device_entries_ex(one, 16000) == [(3, 1.0, [0.0, 0.0, 0.0, 0.0])]
    LA.check_lengths(c, 16000, [15872])
    # chains of the older kinds say what they said
    old = LA.parse_chain([{"kind": "reverberation", "rt60": 0.3}, {"kind": "gaussian_noise", "snr_db": 10}])
    assert LA.device_entries_ex(old, 16000) == [(2, 1.0, [4800.0, 4800.0, -3.0, 0.0]), (0, 1.0, [10.0, 0.0, 0.0, 0.0])]


def test_card_keys_reach_the_embedder(tmp_path):
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        card = yaml.safe_load(f)
    card["loop_attacks"] = [{"kind": "speed_change", "cents": 200.0, "prob": 0.75}, {"kind": "gaussian_noise", "snr_db": 10.0}]
    card["loop_attack_seed"] = 5
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.loop_attacks == [{"kind": "speed_change", "prob": 0.75, "cents": [-200.0, 200.0]},
                                {"kind": "gaussian_noise", "prob": 1.0, "snr_db": 10.0}]
    assert emb.loop_attack_seed == 5
    card["loop_attacks"] = [{"kind": "speed_change", "cents": 200.0}, {"kind": "reverberation", "rt60": 0.2}]
    p.write_text(yaml.safe_dump(card))
    assert load(str(p)) is None


def test_abi_symbols_and_null_handles():
    from aware_amd import _lib
    lib = _lib.load_library()
    assert "aware_speed_change" in _lib.SIGNATURES and hasattr(lib, "aware_speed_change")
    assert "loop_speed_kernels.hip" in _lib.SOURCES
    assert lib.aware_version() == 350
    assert C.sizeof(_lib.LoopAttackEx) == 24 and C.sizeof(_lib.LoopAttack) == 12
    with open(os.path.join(ROOT, "include", "aware_hip.h")) as f:
        hdr = f.read()
    assert "#define AWARE_LOOP_SPEED_CHANGE 3" in hdr
    ent = (_lib.LoopAttackEx * 1)(_lib.LoopAttackEx(3, 0.75, (C.c_float * 4)(-7150.0, 8025.0, 0.0, 0.0)))
    seeds = (C.c_uint32 * 1)(0)
    assert lib.aware_embed_set_loop_attacks_ex(None, ent, 1, seeds, None, 0, None) == -1
    assert lib.aware_embed_loop_attack_workspace_bytes_ex(None, ent, 1) == 0
    old = (_lib.LoopAttack * 1)(_lib.LoopAttack(3, 0.0, 1.0))
    assert lib.aware_embed_set_loop_attacks(None, old, 1, seeds, None, 0, None) == -1
    # the stand-alone entry refuses null pointers and sizes out of range before anything touches a device
    assert lib.aware_speed_change(None, None, None, None, None, None, 1, 16000, None, 0, None) == -1
    p = C.c_void_p(256)                                     # never dereferenced: every call below is refused on its sizes
    q = C.c_void_p(512)
    for B, max_len, adjoint in ((0, 16000, 0), (65536, 16000, 0), (1, 0, 0), (1, (1 << 30) + 1, 0), (1, 16000, 2), (1, 16000, -1)):
        assert lib.aware_speed_change(p, p, p, q, p, p, B, max_len, p, adjoint, None) == -1, (B, max_len, adjoint)
    assert lib.aware_speed_change(p, p, p, p, p, p, 1, 16000, p, 0, None) == -1             # in == out


def test_the_attack_is_registered():
    from aware_amd import attacks as A
    a = A.make_attack("SpeedChange", cents=-84.0)
    assert a.name == "speed_-84.0" and a.cents == -84.0 and a.m == round(65536 * (2 ** (-84.0 / 1200) - 1)) == -3104
    assert A.SpeedChange().name == "speed_50.0" and A.SpeedChange().m == 1920
    assert A.SpeedChange(cents=0.0).m == 0
    assert not any(isinstance(x, A.SpeedChange) for x in A.reference_attack_list())
    assert not any(isinstance(x, A.SpeedChange) for x in A.config3_attack_stack())


# ---- 3. the value claim, on the CPU ---------------------------------------------------------------------------------------------
AWARE_CHAIN = [{"kind": "speed_change", "cents": 200.0, "prob": 0.75}]
RATIOS = [(21, 20), (20, 21), (11, 10), (10, 11)]          # polyphase up / down: -84, +84, -165, +165 cents


def ber_poly(plain, bits, y, up, down):
    return ber(plain, bits, np.stack([O.resample_poly(c.astype(np.float32), up, down) for c in y]))


def snr_db(y, audio):
    """SNR of each watermarked clip against its normalised host, dB."""
    host = audio.astype(np.float64) / (np.abs(audio).max(axis=-1, keepdims=True) + 1e-8)
    host = host[:, :y.shape[-1]]                            # the synthesis keeps whole hops
    return 10 * np.log10((host ** 2).sum(-1) / ((y.astype(np.float64) - host) ** 2).sum(-1))


@pytest.fixture(scope="module")
def value_setup():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    pairs = [make_clip(s, 16000) for s in range(4)]
    audio = np.stack([p[0] for p in pairs])
    bits = np.stack([p[1] for p in pairs])
    wm = np.stack([O.bits_to_bipolar(b) for b in bits]).astype(np.float32)
    plain = O.Embedder()
    y0 = plain.embed(audio, wm)[0].numpy()
    y1 = AttackedEmbedder(AWARE_CHAIN, [0, 1, 2, 3]).embed(audio, wm)[0].numpy()
    return plain, audio, bits, y0, y1


def test_speed_change_in_the_loop_survives_resampling(value_setup):
    """Four 1 s clips, 400 steps, speed_change(+-200 cents, prob 0.75) inside the loop against the oracle's Kaiser polyphase
    resampler (independent of the Catmull-Rom operator) at 21/20, 20/21, 11/10 and 10/11.  Measured with this restatement:
    clean
    0 % both; 101/100 21.25 % plain against 0 %, 100/101 25.00 / 1.25, 21/20 46.25 / 7.50, 20/21 48.75 / 10.00, 11/10 60.00 / 6.25,
    10/11 50.00 / 11.25; mean of the last four 51.25 % against 8.75 %.  SNR against the normalised host: plain 15.97, 14.90,
    16.23, 16.12 dB; speed-aware 15.59, 15.79, 16.22, 15.67 dB.  The margin is wide because the draws are few."""
    plain, audio, bits, y0, y1 = value_setup
    clean0, clean1 = ber(plain, bits, y0), ber(plain, bits, y1)
    print(f"clean BER plain {clean0:.2f} % / speed-aware {clean1:.2f} %")
    r0, r1 = [], []
    for up, down in [(101, 100), (100, 101)] + RATIOS:
        b0, b1 = ber_poly(plain, bits, y0, up, down), ber_poly(plain, bits, y1, up, down)
        print(f"polyphase {up}/{down} ({1200 * np.log2(down / up):+.0f} cents): plain {b0:.2f} % / speed-aware {b1:.2f} %")
        if (up, down) in RATIOS:
            r0.append(b0)
            r1.append(b1)
    m0, m1 = float(np.mean(r0)), float(np.mean(r1))
    print(f"mean of the four wide ratios: plain {m0:.2f} % / speed-aware {m1:.2f} %")
    print("SNR against the normalised host, dB: plain " + ", ".join(f"{v:.2f}" for v in snr_db(y0, audio))
          + " / speed-aware " + ", ".join(f"{v:.2f}" for v in snr_db(y1, audio)))
    assert clean0 == 0.0 and clean1 == 0.0
    assert m0 >= 25.0
    assert m1 <= m0 / 3.0
