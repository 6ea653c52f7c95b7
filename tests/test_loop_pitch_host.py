"""Pitch shift inside the embed loop (EXTENSION): the torch restatement (aware_amd/embedding/loop_attacks.py: pitch_offsets,
pitch_shift, apply_chain) against the composition of the two operators it is made of and against a plain Python loop of its
definition, the gather-form adjoint in the device's order against autograd, the spans the fused kernel stages in LDS, the
validation of the entry and of the chains it may not stand in, the card keys, the C ABI's symbols, and the value claim on the
CPU -- what the fused operator inside the loop buys against the independent phase-vocoder pitch shift, through the oracle's
embed loop.  No GPU."""
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
from test_loop_speed_host import snr_db, speed_adjoint_gather, speed_loop
from test_loop_stretch_host import stretch_adjoint_gather, stretch_loop

PITCH = {"kind": "pitch_shift", "cents": 100.0}
SPEED = {"kind": "speed_change", "cents": 100.0}
STRETCH = {"kind": "time_stretch", "rate": 1.15}
NOISE10 = {"kind": "gaussian_noise", "snr_db": 10.0}
SUP = {"kind": "sample_suppression", "seconds": 0.3}
REVERB = {"kind": "reverberation", "rt60": 0.3}
M_MIN, M_MAX = -13520, 17034                               # the speed offsets of -+400 cents
Q_MIN, Q_MAX = -16384, 21845                               # the stretch's range of offsets
H, N = 256, 1024


def coupled(m):
    """mq and L_u(n) of the speed offset m, in Python integers."""
    R = 65536 + m
    Q = ((1 << 32) + R // 2) // R
    return Q - 65536, lambda n: ((n - 1) << 16) // Q + 1


# ---- 1. the restatement -------------------------------------------------------------------------------------------------------
def test_coupled_rate_over_the_whole_speed_range():
    """Q R is within R / 2 of 2^32 and mq lies inside the stretch's range, for every speed offset; mq = 0 only at m = 0."""
    m = np.arange(M_MIN, M_MAX + 1, dtype=np.int64)
    R = 65536 + m
    Q = ((np.int64(1) << 32) + R // 2) // R
    assert np.all(np.abs(Q * R - (np.int64(1) << 32)) <= R // 2 + 1) and np.all(2 * np.abs(Q * R - (np.int64(1) << 32)) <= R)
    mq = Q - 65536
    assert Q_MIN <= mq.min() and mq.max() <= Q_MAX
    assert (int(mq.min()), int(mq.max())) == (coupled(M_MAX)[0], coupled(M_MIN)[0]) == (-13520, 17034)
    assert np.array_equal(m[mq == 0], [0])
    for v in (M_MIN, -1, 0, 1, 3000, M_MAX):
        assert LA.pitch_offsets(v) == (65536 + v, 65536 + coupled(v)[0])
    assert LA.pitch_offsets(0) == (65536, 65536) and LA.pitch_offsets(1) == (65537, 65535) and LA.pitch_offsets(-1) == (65535, 65537)


@pytest.mark.parametrize("n", [4099, 7937])
@pytest.mark.parametrize("m", [M_MIN, M_MAX, -1, 0, 1, 3000])
def test_pitch_shift_is_the_composition(n, m):
    """Bit for bit in float64: speed_change(time_stretch(x, mq, L_u), m, n), the intermediate at its true stretched length."""
    x = unit_clip(3, n)
    mq, length = coupled(m)
    Lu = length(n)
    assert Lu == LA.stretch_length(n, mq) and abs(Lu - n * (65536 + m) / 65536) < 2
    u = LA.time_stretch(x, mq, Lu)
    assert u.shape == (Lu,)
    for n_out in (n, n - 1000, n + 500):
        z = LA.pitch_shift(x, m, n_out)
        assert z.dtype == torch.float64 and z.shape == (n_out,)
        np.testing.assert_array_equal(z.numpy(), LA.speed_change(u, m, n_out).numpy())
    z = LA.pitch_shift(x, m)
    if m == 0:
        assert z is x                                                                       # the identity returns its input
    else:
        assert z.shape == (n,) and float((z - x).abs().max()) > 1e-3
        live = LA.speed_length(Lu, m)                                                       # outputs whose position lies inside u
        assert abs(live - n) <= 2 and np.all(z.numpy()[live:] == 0.0)                       # the duration stays
    z32 = LA.pitch_shift(x.float(), m)
    assert z32.dtype == torch.float32 and float((z32.double() - z).abs().max()) < 2e-6
    xb = torch.stack([x, -2 * x])                                                           # batched: the last axis; linear
    np.testing.assert_array_equal(LA.pitch_shift(xb, m)[1].numpy(), -2 * z.numpy())


@pytest.mark.parametrize("m", [M_MIN, M_MAX, -1, 1, 3000])
def test_pitch_shift_is_the_definition(m):
    """Against the two sample-by-sample Python loops of the definition, one after the other, exact in float64."""
    n = 4099
    x = unit_clip(3, n)
    mq, length = coupled(m)
    u = stretch_loop(x.numpy(), mq, length(n))
    np.testing.assert_array_equal(LA.pitch_shift(x, m).numpy(), speed_loop(u, m, n))


def test_a_sine_moves_by_the_interval_and_keeps_its_duration():
    """What the operator is for: a 1 kHz sine comes out near 1 kHz times R / 65536, over the clip's whole length.  A plain
    overlap-add does not align the phases of its segments: on the hop grid the stretched signal still advances at the old
    frequency, so its energy lies on the lines f0 Q R / 2^32 + k (sr / 256) R / 65536 (f0 itself to 2^-17, and its images at
    the hop rate after the resampling), weighted by the window's transform around the target f0 R / 65536.  The strongest line
    is therefore within half a line spacing of the target; one bin of the 11904-point spectrum is 1.34 Hz."""
    n, sr = 16000, 16000
    x = torch.sin(2 * np.pi * 1000.0 * torch.arange(n, dtype=torch.float64) / sr)
    one_bin = sr / (n - 4096)
    for cents in (-200.0, 100.0, 400.0):
        m = int(round(65536.0 * (2.0 ** (cents / 1200.0) - 1.0)))
        z = LA.pitch_shift(x, m).numpy()
        spec = np.abs(np.fft.rfft(z[2048:-2048] * np.hanning(n - 4096)))
        peak = float(np.argmax(spec)) * one_bin
        target, spacing = 1000.0 * (65536 + m) / 65536, (sr / 256) * (65536 + m) / 65536
        assert abs(peak - target) <= spacing / 2 + one_bin, (cents, peak)
        k = round((peak - 1000.0) / spacing)
        assert abs(peak - (1000.0 + k * spacing)) <= one_bin, (cents, peak, k)
        assert np.abs(z[-1500:-500]).max() > 0.3                                            # still sounding at the end


def pitch_adjoint_gather(gz, m, n):
    """The adjoint in the order the device takes: gu[k], 0 <= k < L_u, gathers the resampling's inputs in ascending i, then
    gx[j] gathers its frames in ascending t and halves.  Returns gx and the largest count of candidate terms per sample of
    each gather."""
    if m == 0:
        gx = np.zeros(n)
        gx[:min(n, len(gz))] = gz[:n]
        return gx, 0, 0
    mq, length = coupled(m)
    gu, most_i = speed_adjoint_gather(gz, m, length(n))
    gx, most_t = stretch_adjoint_gather(gu, mq, n)
    return gx, most_i, most_t


@pytest.mark.parametrize("m", [-9000, -1, 0, 3, 9000, M_MIN, M_MAX])
def test_gather_adjoint_is_autograd(m):
    """Within 1e-14 of autograd on the restatement.  The kernel's gathers rely on at most six inputs of the resampling per sample
    of gu (four taps at the slowest ratio: ceil(4 * 65536 / 52016)) and at most six frames per input sample (as the stretch)."""
    n = 1531
    for n_out in (n, n - 300, n + 200):
        x = unit_clip(7, n).requires_grad_(True)
        gz = np.cos(0.37 * np.arange(n_out)) * np.linspace(0.2, 1.0, n_out)
        (LA.pitch_shift(x, m, n_out) * torch.from_numpy(gz)).sum().backward()
        gx, most_i, most_t = pitch_adjoint_gather(gz, m, n)
        assert most_i <= 6 and most_t <= 6 and (m != M_MIN or most_i == 6) and (m != M_MAX or most_t == 6)
        grad = x.grad.numpy() if m != 0 or n_out != n else gz
        err = float(np.abs(grad - gx).max())
        assert err <= 1e-14, (m, n_out, err)


SPAN_FWD, SPAN_ADJ, FRAMES = 1296, 3587, 11                 # kPsSpanFwd, kPsSpanAdj, kPsFrames of csrc/loop_pitch_kernels.hip


@pytest.mark.parametrize("m", [M_MIN, M_MAX, -4000, 3000])
def test_the_spans_the_kernel_stages(m):
    """Per tile of 1024 outputs the kernel stages one span of u (forward) or gu (adjoint) in LDS.  The spans it computes hold
    every sample its second phase reads, and stay inside the static bounds its LDS is declared with -- also at the stretch's own
    limits, which the bounds are sized from."""
    n = 7937
    R = 65536 + m
    for mq in (coupled(m)[0], Q_MIN if m > 0 else Q_MAX):
        Q = 65536 + mq
        Lu = ((n - 1) << 16) // Q + 1
        for ta in range(0, n, 1024):
            # forward: taps i0 - 1 .. i0 + 2 of every live output of the tile
            lo = (((ta * R) >> 16) - 1) & ~3
            cnt = (((ta + 1023) * R) >> 16) + 2 - lo + 1
            assert cnt <= SPAN_FWD
            for i in range(ta, min(ta + 1024, n)):
                if i * R <= (Lu - 1) << 16:
                    assert lo <= ((i * R) >> 16) - 1 and ((i * R) >> 16) + 2 < lo + cnt
            # adjoint: the frames t >= -2 with ta - 511 <= a_t <= ta + 1023 + 512, each clipped to the tile
            t = max(-2, -((-(ta - 511) * H) // Q))
            slo, shi, frames = 1 << 40, -1, 0
            while (t * H * Q) >> 16 <= ta + 1023 + 512:
                at = (t * H * Q) >> 16
                slo = min(slo, max(ta - at, -512) + t * H)
                shi = max(shi, min(ta + 1023 - at, 511) + t * H)
                frames += 1
                t += 1
            assert frames <= FRAMES
            slo, shi = max(slo, 0), min(shi, Lu - 1)
            lo = slo & ~3
            assert shi - lo + 1 <= SPAN_ADJ
            for j in range(ta, min(ta + 1024, n), 7):
                t = max(-2, -((-(j - 511) * H) // Q))
                while (t * H * Q) >> 16 <= j + 512:
                    o = j - ((t * H * Q) >> 16) + t * H
                    assert not 0 <= o < Lu or lo <= o <= shi
                    t += 1


# ---- 2. the chain -----------------------------------------------------------------------------------------------------------------
def drawn(chain, seed, step, j=0):
    e = LA.parse_chain(chain)[j]
    return LA.speed_offset(LA.entry_draw(seed, step, j)[3], *LA.speed_range(e))


def test_draws_differ_between_steps_and_clips():
    ms = {(sd, s): drawn([PITCH], sd, s) for sd in range(4) for s in range(8)}
    assert len(set(ms.values())) >= 30                                                    # 32 draws on 7575 values
    x = torch.stack([unit_clip(1), unit_clip(1)])
    z0, z1 = LA.apply_chain(x, [PITCH], [0, 1], 0), LA.apply_chain(x, [PITCH], [0, 1], 1)
    assert float((z0[0] - z0[1]).abs().max()) > 0.1 and float((z0[0] - z1[0]).abs().max()) > 0.1
    np.testing.assert_array_equal(LA.apply_chain(x, [PITCH], [0, 1], 0).numpy(), z0.numpy())    # reproducible
    np.testing.assert_array_equal(z0[1].numpy(), LA.pitch_shift(x[1], ms[(1, 0)]).numpy())
    # the entry's index keys the draw
    shifted = LA.apply_chain(x[:1], [dict(NOISE10, prob=0.0), PITCH], [0], 0)[0]
    np.testing.assert_array_equal(shifted.numpy(), LA.pitch_shift(x[0], drawn([NOISE10, PITCH], 0, 0, 1)).numpy())
    assert drawn([NOISE10, PITCH], 0, 0, 1) != ms[(0, 0)]
    # the draw is the speed change's: the same entry index, seed and step give the same offset
    assert drawn([SPEED], 2, 5) == ms[(2, 5)]


def test_probability_and_identity():
    x = unit_clip(4)[None]
    for step in range(5):
        np.testing.assert_array_equal(LA.apply_chain(x, [dict(PITCH, prob=0.0)], [9], step).numpy(), x.numpy())
    fired = sum(int(not torch.equal(LA.apply_chain(x[:, :2048], [dict(PITCH, prob=0.75)], [2], s), x[:, :2048]))
                for s in range(400))
    assert 0.68 * 400 < fired < 0.82 * 400, fired                                         # 0.75 +- 3 sigma of 400 draws


def test_order_with_noise_and_suppression():
    x = unit_clip(6)[None]
    e = LA.parse_chain([{"kind": "pitch_shift", "cents": [150.0, 300.0]}])[0]
    m = drawn([e], 1, 0)
    res = LA.apply_chain(x, [e], [1], 0)[0]
    np.testing.assert_array_equal(res.numpy(), LA.pitch_shift(x[0], m).numpy())
    # noise behind the entry: its sigma comes from the shifted signal
    both = LA.apply_chain(x, [e, NOISE10], [1], 0)[0]
    sigma = np.sqrt(float((res ** 2).mean()) / 10.0)
    np.testing.assert_allclose((both - res).numpy(), sigma * LA.normal_draws(16000, 1, 0, 1), atol=1e-12)
    # noise in front: it is shifted too (the offset is entry 1's)
    front = LA.apply_chain(x, [NOISE10, e], [1], 0)[0]
    noisy = LA.apply_chain(x, [NOISE10], [1], 0)[0]
    m1 = drawn([NOISE10, e], 1, 0, 1)
    np.testing.assert_array_equal(front.numpy(), LA.pitch_shift(noisy, m1).numpy())
    # a suppression behind the entry is where it was drawn; in front, the gap keeps its place in time (the duration stays) and
    # is blurred by the window at its edges only
    b = LA.apply_chain(x, [e, SUP], [1], 0)[0]
    s_b = LA.suppression_start(LA.entry_draw(1, 0, 1)[1], 16000, 4800)
    assert float(b[s_b:s_b + 4800].abs().max()) == 0.0
    a = LA.apply_chain(x, [SUP, e], [1], 0)[0]
    s_a = LA.suppression_start(LA.entry_draw(1, 0, 0)[1], 16000, 4800)
    inner = slice(s_a + 1100, s_a + 4800 - 1100)
    assert float(a[inner].abs().max()) == 0.0 and float(a[s_a - 1200:s_a - 100].abs().max()) > 0.0
    # all four places
    full = LA.apply_chain(x, [SUP, NOISE10, e, NOISE10], [1], 3)
    assert full.shape == x.shape


def test_ragged_lists():
    clips = [unit_clip(1, 7937), unit_clip(2, 40000)]
    out = LA.apply_chain(clips, [PITCH], [4, 5], 2)
    assert isinstance(out, list) and [len(o) for o in out] == [7937, 40000]
    np.testing.assert_array_equal(out[1].numpy(), LA.apply_chain(clips[1][None], [PITCH], [5], 2)[0].numpy())


# ---- 3. validation, card keys, ABI ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [
    [{"kind": "pitch"}],
    [{"kind": "pitch_shift"}],
    [{"kind": "pitch_shift", "prob": 0.5}],
    [{"kind": "pitch_shift", "cents": 0.0}],
    [{"kind": "pitch_shift", "cents": -50.0}],
    [{"kind": "pitch_shift", "cents": [50.0, -50.0]}],
    [{"kind": "pitch_shift", "cents": 400.5}],
    [{"kind": "pitch_shift", "cents": [-401.0, 0.0]}],
    [{"kind": "pitch_shift", "cents": [0.0, 400.001]}],
    [{"kind": "pitch_shift", "cents": float("nan")}],
    [{"kind": "pitch_shift", "cents": float("inf")}],
    [{"kind": "pitch_shift", "cents": [float("nan"), 10.0]}],
    [{"kind": "pitch_shift", "cents": [-10.0, float("inf")]}],
    [{"kind": "pitch_shift", "cents": [-10.0, 0.0, 10.0]}],
    [{"kind": "pitch_shift", "cents": "high"}],
    [{"kind": "pitch_shift", "cents": 100.0, "prob": 1.5}],
    [{"kind": "pitch_shift", "cents": 100.0, "prob": -0.1}],
    [{"kind": "pitch_shift", "cents": 100.0, "rate": 1.1}],
    [{"kind": "pitch_shift", "cents": 100.0, "rt60": 0.3}],
    [{"kind": "pitch_shift", "cents": 100.0, "seconds": 0.3}],
    [{"kind": "pitch_shift", "cents": [0.001, 0.002]}],                                  # no offset inside: m_lo = 1 > m_hi = 0
    [PITCH, {"kind": "pitch_shift", "cents": 50.0}],
    [PITCH, NOISE10, {"kind": "pitch_shift", "cents": 50.0}],
    [PITCH, REVERB], [REVERB, PITCH], [REVERB, NOISE10, PITCH], [PITCH, SUP, REVERB],
    [PITCH, SPEED], [SPEED, PITCH], [SPEED, NOISE10, PITCH], [PITCH, NOISE10, SPEED],
    [PITCH, STRETCH], [STRETCH, PITCH], [STRETCH, NOISE10, PITCH], [PITCH, SUP, STRETCH],
    [STRETCH, SPEED, PITCH], [PITCH, STRETCH, SPEED],
    [PITCH, NOISE10, SUP, NOISE10, SUP],
])
def test_invalid_chains_are_refused(chain):
    with pytest.raises(ValueError):
        LA.parse_chain(chain)
    from aware_amd.embedding import AWAREEmbedder
    with pytest.raises(ValueError):
        AWAREEmbedder(loss="push_extremes", verbose=False, loop_attacks=chain)


def test_parse_fills_defaults():
    assert LA.KINDS["pitch_shift"] == 5 and LA.KINDS["time_stretch"] == 4 and LA.KINDS["speed_change"] == 3 and LA.MAX_CENTS == 400.0
    c = LA.parse_chain([{"kind": "sample_suppression", "seconds": 0.5}, {"kind": "gaussian_noise", "snr_db": 20},
                        {"kind": "pitch_shift", "cents": 100}, {"kind": "gaussian_noise", "snr_db": 10}])
    assert c == [{"kind": "sample_suppression", "prob": 1.0, "seconds": 0.5},
                 {"kind": "gaussian_noise", "prob": 1.0, "snr_db": 20.0},
                 {"kind": "pitch_shift", "prob": 1.0, "cents": [-100.0, 100.0]},
                 {"kind": "gaussian_noise", "prob": 1.0, "snr_db": 10.0}]
    assert LA.parse_chain(c) == c                                                          # a parsed chain parses to itself
    assert LA.device_entries_ex(c, 16000) == [(1, 1.0, [8000.0, 0.0, 0.0, 0.0]), (0, 1.0, [20.0, 0.0, 0.0, 0.0]),
                                              (5, 1.0, [-3678.0, 3896.0, 0.0, 0.0]), (0, 1.0, [10.0, 0.0, 0.0, 0.0])]
    r = LA.parse_chain([{"kind": "pitch_shift", "cents": (-50.0, 120.0), "prob": 0.75}])
    assert r == [{"kind": "pitch_shift", "prob": 0.75, "cents": [-50.0, 120.0]}]
    p = 0.75
    m_lo, m_hi = LA.speed_range(r[0])
    assert LA.device_entries_ex(r, 16000) == [(5, p, [float(m_lo), float(m_hi), 0.0, 0.0])]
    assert (m_lo, m_hi) == LA.speed_range(LA.parse_chain([{"kind": "speed_change", "cents": [-50.0, 120.0]}])[0])
    assert LA.device_entries_ex(LA.parse_chain([{"kind": "pitch_shift", "cents": 400.0}]), 16000) == \
        [(5, 1.0, [float(M_MIN), float(M_MAX), 0.0, 0.0])]
    one = LA.parse_chain([{"kind": "pitch_shift", "cents": [0.0, 0.0]}])                   # one value: the identity
    assert LA.device_entries_ex(one, 16000) == [(5, 1.0, [0.0, 0.0, 0.0, 0.0])]
    LA.check_lengths(c, 16000, [15872])
    with pytest.raises(ValueError):
        LA.check_lengths(c, 16000, [7936])                                                 # the suppression does not fit
    # chains of the older kinds say what they said
    old = LA.parse_chain([{"kind": "speed_change", "cents": 200.0}, {"kind": "gaussian_noise", "snr_db": 10}])
    assert old == [{"kind": "speed_change", "prob": 1.0, "cents": [-200.0, 200.0]}, {"kind": "gaussian_noise", "prob": 1.0, "snr_db": 10.0}]
    assert LA.device_entries_ex(old, 16000) == [(3, 1.0, [-7150.0, 8025.0, 0.0, 0.0]), (0, 1.0, [10.0, 0.0, 0.0, 0.0])]
    pair = LA.parse_chain([{"kind": "time_stretch", "rate": 1.25}, {"kind": "speed_change", "cents": 100}])
    assert LA.device_entries_ex(pair, 16000) == [(4, 1.0, [-13107.0, 16384.0, 0.0, 0.0]), (3, 1.0, [-3678.0, 3896.0, 0.0, 0.0])]
    rv = LA.parse_chain([{"kind": "reverberation", "rt60": [0.1, 0.5]}])
    assert LA.device_entries_ex(rv, 16000) == [(2, 1.0, [1600.0, 8000.0, -3.0, 0.0])]


def test_card_keys_reach_the_embedder(tmp_path):
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        card = yaml.safe_load(f)
    card["loop_attacks"] = [{"kind": "gaussian_noise", "snr_db": 20.0}, {"kind": "pitch_shift", "cents": 150.0, "prob": 0.75}]
    card["loop_attack_seed"] = 5
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.loop_attacks == [{"kind": "gaussian_noise", "prob": 1.0, "snr_db": 20.0},
                                {"kind": "pitch_shift", "prob": 0.75, "cents": [-150.0, 150.0]}]
    assert emb.loop_attack_seed == 5
    card["loop_attacks"] = [{"kind": "pitch_shift", "cents": 100.0}, {"kind": "speed_change", "cents": 100.0}]
    p.write_text(yaml.safe_dump(card))
    assert load(str(p)) is None


def test_abi_symbols_and_null_handles():
    from aware_amd import _lib
    lib = _lib.load_library()
    assert "aware_pitch_shift_ola" in _lib.SIGNATURES and hasattr(lib, "aware_pitch_shift_ola")
    assert _lib.SIGNATURES["aware_pitch_shift_ola"] == _lib.SIGNATURES["aware_speed_change"]
    assert "loop_pitch_kernels.hip" in _lib.SOURCES
    assert lib.aware_version() == 350
    assert C.sizeof(_lib.LoopAttackEx) == 24 and C.sizeof(_lib.LoopAttack) == 12
    with open(os.path.join(ROOT, "include", "aware_hip.h")) as f:
        hdr = f.read()
    assert "#define AWARE_LOOP_PITCH_SHIFT 5" in hdr and "int aware_pitch_shift_ola(" in hdr
    ent = (_lib.LoopAttackEx * 1)(_lib.LoopAttackEx(5, 0.75, (C.c_float * 4)(-3678.0, 3896.0, 0.0, 0.0)))
    seeds = (C.c_uint32 * 1)(0)
    assert lib.aware_embed_set_loop_attacks_ex(None, ent, 1, seeds, None, 0, None) == -1
    assert lib.aware_embed_loop_attack_workspace_bytes_ex(None, ent, 1) == 0
    old = (_lib.LoopAttack * 1)(_lib.LoopAttack(5, 0.0, 1.0))                               # kind 5 through the older call
    assert lib.aware_embed_set_loop_attacks(None, old, 1, seeds, None, 0, None) == -1
    # the stand-alone entry refuses null pointers and sizes out of range before anything touches a device
    assert lib.aware_pitch_shift_ola(None, None, None, None, None, None, 1, 16000, None, 0, None) == -1
    p = C.c_void_p(256)                                     # never dereferenced: every call below is refused on its sizes
    q = C.c_void_p(512)
    for B, max_len, adjoint in ((0, 16000, 0), (65536, 16000, 0), (1, 0, 0), (1, (1 << 30) + 1, 0), (1, 16000, 2), (1, 16000, -1)):
        assert lib.aware_pitch_shift_ola(p, p, p, q, p, p, B, max_len, p, adjoint, None) == -1, (B, max_len, adjoint)
    for hole in range(6):                                   # each pointer in turn
        args = [p, p, p, q, p, p]
        args[hole] = None
        assert lib.aware_pitch_shift_ola(*args, 1, 16000, p, 0, None) == -1
    assert lib.aware_pitch_shift_ola(p, p, p, q, p, p, 1, 16000, None, 0, None) == -1
    assert lib.aware_pitch_shift_ola(p, p, p, p, p, p, 1, 16000, p, 0, None) == -1          # in == out


def test_the_attack_is_registered():
    from aware_amd import attacks as A
    assert "OverlapAddPitchShift" in A.ATTACKS
    a = A.make_attack("OverlapAddPitchShift", cents=-100.0)
    assert a.name == "ola_ps_-100.0" and a.cents == -100.0 and a.m == round(65536 * (2 ** (-100 / 1200) - 1)) == -3678
    assert A.OverlapAddPitchShift().name == "ola_ps_50.0" and A.OverlapAddPitchShift().m == 1920
    assert A.OverlapAddPitchShift(cents=0.0).m == 0
    assert not any(isinstance(x, A.OverlapAddPitchShift) for x in A.reference_attack_list())
    assert not any(isinstance(x, A.OverlapAddPitchShift) for x in A.config3_attack_stack())
    assert A.make_attack("PitchShift", cents=50).name != A.OverlapAddPitchShift().name     # the phase vocoder stays what it is
    assert not isinstance(A.make_attack("PitchShift", cents=50), A.OverlapAddPitchShift)


# ---- 4. the value claim, on the CPU ---------------------------------------------------------------------------------------------
AWARE_CHAIN = [{"kind": "pitch_shift", "cents": 150.0, "prob": 0.75}]       # +-150 cents: the lower mean of the two ranges tried
RATES = [0.9, 0.95, 1.05, 1.1]
CENTS = [-100, -50, 50, 100]


def test_pitch_shift_in_the_loop_against_the_phase_vocoder():
    """Four 1 s clips, 400 steps, card settings: plain, and pitch_shift(+-150 cents, prob 0.75) inside the loop, against the
    oracle's phase-vocoder pitch shift (independent of the overlap-add operator) at -+50 and -+100 cents, and against its time
    stretch at 0.9, 0.95, 1.05 and 1.1.  Measured with this restatement, plain / pitch-aware BER in %: clean 0 / 0; pitch shift by
    -100 cents 56.25 / 35.00, -50 cents 52.50 / 38.75, +50 cents 48.75 / 51.25, +100 cents 50.00 / 46.25, mean 51.88 / 42.81; phase
    vocoder stretch at 0.9 28.75 / 27.50, 0.95 32.50 / 28.75, 1.05 32.50 / 16.25, 1.1 33.75 / 36.25, mean 31.88 / 27.19.  SNR
    against the normalised host, dB: plain 15.97, 14.90, 16.23, 16.12; pitch-aware 15.38, 15.66, 16.13, 15.47.  With +-100 cents
    in the loop instead: clean 0, pitch shift 42.50, 46.25, 47.50, 45.00, mean 45.31; stretch 22.50, 32.50, 16.25, 32.50, mean
    25.94; SNR 15.81, 15.15, 15.35, 15.24.  The pitch-aware mean is above two thirds of the plain one (34.58 %) with either range,
    so nothing is asserted about it: DESIGN.md section 19, "Limitation"."""
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    pairs = [make_clip(s, 16000) for s in range(4)]
    audio = np.stack([p[0] for p in pairs])
    bits = np.stack([p[1] for p in pairs])
    wm = np.stack([O.bits_to_bipolar(b) for b in bits]).astype(np.float32)
    plain = O.Embedder()
    ys = {"plain": plain.embed(audio, wm)[0].numpy(),
          "pitch-aware": AttackedEmbedder(AWARE_CHAIN, [0, 1, 2, 3]).embed(audio, wm)[0].numpy()}
    names = list(ys)
    clean = {k: ber(plain, bits, y) for k, y in ys.items()}
    print("clean BER: " + " / ".join(f"{k} {clean[k]:.2f} %" for k in names))
    ps = {k: [ber(plain, bits, np.stack([O.pitch_shift_attack(c.astype(np.float32), ct) for c in ys[k]])) for ct in CENTS] for k in names}
    for i, c in enumerate(CENTS):
        print(f"pitch shift by {c:+d} cents: " + " / ".join(f"{k} {ps[k][i]:.2f} %" for k in names))
    st = {k: [ber(plain, bits, np.stack([O.time_stretch_attack(c.astype(np.float32), r) for c in ys[k]])) for r in RATES] for k in names}
    for i, r in enumerate(RATES):
        print(f"phase vocoder stretch at {r}: " + " / ".join(f"{k} {st[k][i]:.2f} %" for k in names))
    mp = {k: float(np.mean(ps[k])) for k in names}
    ms = {k: float(np.mean(st[k])) for k in names}
    print("mean over the four pitch shifts: " + " / ".join(f"{k} {mp[k]:.2f} %" for k in names))
    print("mean over the four rates: " + " / ".join(f"{k} {ms[k]:.2f} %" for k in names))
    for k in names:
        print(f"SNR against the normalised host, dB, {k}: " + ", ".join(f"{v:.2f}" for v in snr_db(ys[k], audio)))
    assert all(clean[k] == 0.0 for k in names)
    assert mp["plain"] >= 25.0
