"""The time warp inside the embed loop (EXTENSION, chain kind 11): the restatement of aware_amd/embedding/loop_attacks.py
(warp_range, warp_draw, warp_rates, warp_table, warp_positions, time_warp, time_warp_adjoint, apply_chain) against a plain loop of
Python integers over the definition, its adjoint against the inner product, autograd and gradcheck, its draws and its place in a
chain and a mixture, the parser in Python and in C (csrc/loop_chain.hpp through tests/host_sim/loop_chain_check on the CPU), the
card keys, the ABI, and the value claim on the CPU: what the kind buys against wow and flutter, a speed that moves inside the
clip, through the oracle's embed loop.  No GPU."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, make_clip  # noqa: F401
from aware_amd.embedding import loop_attacks as LA
from test_loop_attacks_host import (AttackedEmbedder, _chain_case, _dims_case, _golden, _mixture_case, ber, unit_clip,  # noqa: F401
                                    value_setup)
from test_loop_gain_host import snr_db

AWARE_CHAIN = [{"kind": "time_warp", "depth": 0.04, "period": [0.032, 0.512], "prob": 0.75}]      # the card's commented line
SPEED_CHAIN = [{"kind": "speed_change", "cents": 60.0, "prob": 0.75}]
TW = {"kind": "time_warp", "depth": 0.04, "period": [0.032, 0.512]}
NOISE = {"kind": "gaussian_noise", "snr_db": 10.0}
SUP = {"kind": "sample_suppression", "seconds": 0.3}
FIL = {"kind": "band_filter", "response": "lowpass", "freq": 1000.0}
EXC = {"kind": "excerpt", "seconds": 0.5}
SIZES, EXPS, DEPTHS = (513, 4099, 7937), (8, 10, 14), (1, 6553)


# ---- 1. the model -------------------------------------------------------------------------------------------------------------------
def plain_table(e, rates):
    """R_k and A(k) from the definition, in Python's integers (>> floors, as an arithmetic shift does)."""
    P = 1 << e
    R = [65536 + int(m) for m in rates]
    A = [0]
    for k in range(len(R) - 1):
        A.append(A[k] + P * R[k] + (((R[k + 1] - R[k]) * P) >> 1))
    return R, A


def plain_positions(n, e, ph, rates):
    """p_i = Pos(i + ph) - Pos(ph), sample by sample."""
    P = 1 << e
    R, A = plain_table(e, rates)

    def pos(u):
        k, t = u >> e, u & (P - 1)
        return A[k] + t * R[k] + (((R[k + 1] - R[k]) * t * t) >> (e + 1))

    return [pos(i + ph) - pos(ph) for i in range(n)]


def plain_warp(x, p):
    """z[i] = the Catmull-Rom tap at p_i, in Python floats; zero past the clip's last sample."""
    n = len(x)
    at = lambda i: float(x[i]) if 0 <= i < n else 0.0
    out = []
    for pi in p:
        if pi > (n - 1) << 16:
            out.append(0.0)
            continue
        i0, f = pi >> 16, (pi & 0xFFFF) / 65536.0
        w = (((-f + 2) * f - 1) * f / 2, ((3 * f - 5) * f * f + 2) / 2, ((-3 * f + 4) * f + 1) * f / 2, (f - 1) * f * f / 2)
        out.append(w[0] * at(i0 - 1) + w[1] * at(i0) + w[2] * at(i0 + 1) + w[3] * at(i0 + 2))
    return out


def drawn_rates(seed, n, e, D):
    return LA.warp_rates(seed, 3, 1, LA.warp_breakpoints(n, e), D)


@pytest.mark.parametrize("n", SIZES)
def test_positions_are_the_definition(n):
    """warp_positions and warp_table against the plain loop at e = 8, 10 and 14 (2^14 is longer than every clip here: one segment),
    both ends of the phase and both ends of the depth; strictly increasing with steps inside [R_min - 1, R_max + 1]; continuous at
    every breakpoint: the segment's formula at t = P is the next A."""
    for e in EXPS:
        P = 1 << e
        for ph in (0, P - 1):
            for D in DEPTHS:
                m = drawn_rates(n + e, n, e, D)
                assert len(m) == ((n + P - 1) >> e) + 2 and m.dtype == np.int64 and np.all(np.abs(m) <= D)
                p = LA.warp_positions(n, e, ph, m)
                assert p.dtype == np.int64 and p[0] == 0
                assert p.tolist() == plain_positions(n, e, ph, m), (e, ph, D)
                d = np.diff(p)
                assert d.min() >= 65536 - D - 1 and d.max() <= 65536 + D + 1 and d.min() > 0
                R, A = LA.warp_table(m, e)
                Rp, Ap = plain_table(e, m)
                assert R.tolist() == Rp and A.tolist() == Ap
                for k in range(len(m) - 1):
                    assert Ap[k] + P * Rp[k] + (((Rp[k + 1] - Rp[k]) * P * P) >> (e + 1)) == Ap[k + 1]
    if n == 7937:
        assert D == 6553 and len(set(np.diff(p).tolist())) > 100                          # the rate does move
    with pytest.raises(ValueError):
        LA.warp_positions(n, 8, 256, np.zeros(100, dtype=np.int64))                        # ph outside [0, P)
    with pytest.raises(ValueError):
        LA.warp_positions(n, 7, 0, np.zeros(100, dtype=np.int64))
    with pytest.raises(ValueError):
        LA.warp_positions(n, 8, 0, np.zeros(LA.warp_breakpoints(n, 8) - 1, dtype=np.int64))
    with pytest.raises(ValueError):
        LA.warp_positions(n, 8, 0, np.full(LA.warp_breakpoints(n, 8), 6554))


def test_draws_are_the_definition():
    """m_k = -D + ((w_k (2 D + 1)) >> 32) from counter (k // 4, step, 20 + j, 0): both ends are reached, the streams of steps,
    entries and clips differ, and the words do not collide with the envelope's (16 + j)."""
    for D in DEPTHS:
        m = LA.warp_rates(7, 5, 2, 4001, D)
        ctr = np.zeros((1001, 4), dtype=np.uint64)
        ctr[:, 0], ctr[:, 1], ctr[:, 2] = np.arange(1001), 5, 22
        w = LA.philox4x32(ctr, (7, 0x5EED)).reshape(-1)[:4001]
        assert m.tolist() == [-D + ((int(v) * (2 * D + 1)) >> 32) for v in w]
        assert -D <= m.min() <= -0.99 * D and 0.99 * D <= m.max() <= D                 # 4001 draws over 3 or 13107 values
    a = LA.warp_rates(7, 5, 2, 64, 6553)
    assert not np.array_equal(a, LA.warp_rates(7, 6, 2, 64, 6553)) and not np.array_equal(a, LA.warp_rates(7, 5, 1, 64, 6553))
    assert not np.array_equal(a, LA.warp_rates(8, 5, 2, 64, 6553))
    assert np.array_equal(LA.warp_rates(7 + (1 << 32), 5, 2, 64, 6553), a)                 # the seed is 32 bits wide
    e = LA.parse_chain([TW])[0]
    assert LA.warp_range(e, 16000) == (9, 13, 2621)
    seen = set()
    for seed in range(4):
        for step in range(40):
            r = LA.entry_draw(seed, step, 0)
            ex, ph = LA.warp_draw(e, r, 16000)
            assert ex == 9 + ((int(r[2]) * 5) >> 32) and ph == (int(r[1]) << ex) >> 32 and 0 <= ph < (1 << ex)
            seen.add(ex)
    assert seen == {9, 10, 11, 12, 13}
    lo, hi = np.array([0, 0, 0, 0], dtype=np.uint32), np.array([0, 0xFFFFFFFF, 0xFFFFFFFF, 0], dtype=np.uint32)
    assert LA.warp_draw(e, lo, 16000) == (9, 0) and LA.warp_draw(e, hi, 16000) == (13, 8191)


@pytest.mark.parametrize("n", SIZES)
def test_time_warp_is_the_definition(n):
    x = unit_clip(3, n)
    for e in EXPS:
        for ph in (0, (1 << e) - 1):
            m = drawn_rates(n, n, e, 6553)
            z = LA.time_warp(x, e, ph, m)
            assert z.dtype == torch.float64 and z.shape == (n,)
            np.testing.assert_allclose(z.numpy(), np.array(plain_warp(x.numpy(), plain_positions(n, e, ph, m))), rtol=0, atol=1e-14)
            assert LA.time_warp(x.float(), e, ph, m).dtype == torch.float32
    xb, m = torch.stack([x, -2 * x]), drawn_rates(n, n, 8, 6553)                           # the operator acts on the last axis
    np.testing.assert_allclose(LA.time_warp(xb, 8, 5, m)[1].numpy(), -2 * LA.time_warp(x, 8, 5, m).numpy(), rtol=0, atol=1e-14)


@pytest.mark.parametrize("n", SIZES)
def test_constant_rates(n):
    """All-zero offsets are the identity, bit for bit and in both directions; all +D is the speed change at m = D, which ends in
    zeros; all -D is the speed change at m = -D, which never reaches the clip's end."""
    x = unit_clip(4, n)
    for e in EXPS:
        K = LA.warp_breakpoints(n, e)
        for ph in (0, (1 << e) - 1):
            zero = np.zeros(K, dtype=np.int64)
            assert LA.time_warp(x, e, ph, zero) is x and LA.time_warp_adjoint(x, e, ph, zero) is x
            assert LA.warp_positions(n, e, ph, zero).tolist() == [i << 16 for i in range(n)]
            for D in DEPTHS:
                for sign in (1, -1):
                    m = np.full(K, sign * D, dtype=np.int64)
                    assert LA.warp_positions(n, e, ph, m).tolist() == [i * (65536 + sign * D) for i in range(n)]
                    for dt in (torch.float64, torch.float32):
                        z = LA.time_warp(x.to(dt), e, ph, m)
                        assert torch.equal(z, LA.speed_change(x.to(dt), sign * D))
            fast = LA.time_warp(x, e, ph, np.full(K, 6553, dtype=np.int64))
            dead = n - 1 - ((n - 1) << 16) // (65536 + 6553)                                # outputs past the last sample
            assert dead >= 46 and torch.count_nonzero(fast[n - dead:]) == 0 and fast[n - dead - 1] != 0
            slow = LA.time_warp(x, e, ph, np.full(K, -6553, dtype=np.int64))
            assert (LA.warp_positions(n, e, ph, np.full(K, -6553))[-1] >> 16) == ((n - 1) * (65536 - 6553)) >> 16 < n - 46
            assert slow[-1] != 0


@pytest.mark.parametrize("n", SIZES)
def test_adjoint_is_the_transpose(n):
    """<z, w> = <x, adjoint(w)> in float64, and the adjoint is what autograd gives."""
    x = unit_clip(7, n)
    w = torch.from_numpy(np.cos(0.37 * np.arange(n)) * np.linspace(0.2, 1.0, n))
    for e in EXPS:
        for ph in (0, (1 << e) - 1):
            for D in DEPTHS:
                m = drawn_rates(n + D, n, e, D)
                z, gx = LA.time_warp(x, e, ph, m), LA.time_warp_adjoint(w, e, ph, m)
                lhs, rhs = float((z * w).sum()), float((x * gx).sum())
                assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (e, ph, D, lhs, rhs)
                xg = x.clone().requires_grad_(True)
                (LA.time_warp(xg, e, ph, m) * w).sum().backward()
                np.testing.assert_allclose(xg.grad.numpy(), gx.numpy(), rtol=0, atol=1e-13)
    clips = [unit_clip(1, 1025), unit_clip(2, 4099)]
    ms = [drawn_rates(b, len(c), 8 + 2 * b, 3000) for b, c in enumerate(clips)]
    out = LA.time_warp(clips, [8, 10], [3, 1000], ms)
    back = LA.time_warp_adjoint(clips, [8, 10], [3, 1000], ms)
    assert isinstance(out, list) and [len(o) for o in out] == [1025, 4099] and [len(o) for o in back] == [1025, 4099]
    assert torch.equal(out[1], LA.time_warp(clips[1], 10, 1000, ms[1])) and torch.equal(back[1], LA.time_warp_adjoint(clips[1], 10, 1000, ms[1]))


def test_gradcheck():
    x = unit_clip(5, 300).requires_grad_(True)
    for ph, D in ((0, 6553), (255, 6553), (17, 1)):
        m = drawn_rates(ph, 300, 8, D)
        assert torch.autograd.gradcheck(lambda v: LA.time_warp(v, 8, ph, m), (x,), eps=1e-6, atol=1e-8)


# ---- 2. in a chain ------------------------------------------------------------------------------------------------------------------
def host_warp(x, entry, seed, step, j, sr=16000):
    """The entry's warp of x for this clip, step and place in the chain, from the parts."""
    e, ph = LA.warp_draw(entry, LA.entry_draw(seed, step, j), sr)
    return LA.time_warp(x, e, ph, LA.warp_rates(seed, step, j, LA.warp_breakpoints(x.shape[-1], e), LA.warp_range(entry, sr)[2]))


def test_probability_and_identity():
    x = unit_clip(4, 15872)[None]
    e = LA.parse_chain([TW])[0]
    for step in range(5):
        assert torch.equal(LA.apply_chain(x, [dict(TW, prob=0.0)], [9], step), x)
        assert torch.equal(LA.apply_chain(x, [dict(TW, prob=1.0)], [9], step)[0], host_warp(x[0], e, 9, step, 0))
    fired = sum(int(not torch.equal(LA.apply_chain(x, [dict(TW, prob=0.75)], [2], s), x)) for s in range(200))
    assert fired == sum(int(LA.fires(LA.entry_draw(2, s, 0)[0], 0.75)) for s in range(200))
    assert abs(fired - 150) <= 3 * math.sqrt(200 * 0.75 * 0.25), fired                      # 0.75 +- 3 sigma of 200 draws
    outs = [LA.apply_chain(x, [TW], [sd], st)[0] for sd, st in ((1, 0), (1, 1), (2, 0))]
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])          # steps and clips draw their own


def test_a_scalar_period():
    p = LA.parse_chain([{"kind": "time_warp", "depth": 0.02, "period": 0.064}])[0]
    assert p == {"kind": "time_warp", "prob": 1.0, "period": 0.064, "depth": 0.02} and LA.warp_range(p, 16000) == (10, 10, 1310)
    assert LA.warp_range(LA.parse_chain([{"kind": "time_warp", "depth": 0.02, "period": 0.05}])[0], 16000)[:2] == (10, 10)      # 800: the nearest
    assert LA.warp_range(LA.parse_chain([{"kind": "time_warp", "depth": 0.02, "period": 0.1}])[0], 16000)[:2] == (11, 11)      # 1600
    for step in range(6):
        assert LA.warp_draw(p, LA.entry_draw(3, step, 0), 16000)[0] == 10


def test_order_with_noise_and_suppression():
    x = unit_clip(6, 15872)[None]
    e = LA.parse_chain([TW])[0]
    res = LA.apply_chain(x, [e], [1], 0)[0]
    assert torch.equal(res, host_warp(x[0], e, 1, 0, 0))
    # noise behind it: its sigma comes from the warped signal
    both = LA.apply_chain(x, [e, NOISE], [1], 0)[0]
    sigma = np.sqrt(float((res ** 2).mean()) / 10.0)
    np.testing.assert_allclose((both - res).numpy(), sigma * LA.normal_draws(15872, 1, 0, 1), atol=1e-12)
    # noise in front: it is warped with the clip (the draw and the rates are entry 1's)
    front = LA.apply_chain(x, [NOISE, e], [1], 0)[0]
    noisy = LA.apply_chain(x, [NOISE], [1], 0)[0]
    assert torch.equal(front, host_warp(noisy, e, 1, 0, 1)) and not torch.equal(front, host_warp(noisy, e, 1, 0, 0))
    # a suppression in front is warped too: the hole moves and keeps its zeros but for the taps at its edges
    sup = LA.apply_chain(x, [SUP, e], [1], 0)[0]
    assert torch.equal(sup, host_warp(LA.apply_chain(x, [SUP], [1], 0)[0], e, 1, 0, 1))
    assert int((sup == 0).sum()) > 4000
    # ragged lists keep their container
    clips = [unit_clip(1, 7936), unit_clip(2, 40192)]
    out = LA.apply_chain(clips, [e], [4, 5], 2)
    assert isinstance(out, list) and [len(o) for o in out] == [7936, 40192]
    assert torch.equal(out[1], LA.apply_chain(clips[1][None], [e], [5], 2)[0])
    assert torch.equal(out[0], host_warp(clips[0], e, 4, 2, 0))


def test_the_chain_is_differentiable_with_the_rates_detached():
    x = unit_clip(8, 4096)[None].clone().requires_grad_(True)
    w = torch.from_numpy(np.sin(0.11 * np.arange(4096)))
    (LA.apply_chain(x, [TW], [3], 1)[0] * w).sum().backward()
    e = LA.parse_chain([TW])[0]
    ex, ph = LA.warp_draw(e, LA.entry_draw(3, 1, 0), 16000)
    gx = LA.time_warp_adjoint(w, ex, ph, LA.warp_rates(3, 1, 0, LA.warp_breakpoints(4096, ex), 2621))
    np.testing.assert_allclose(x.grad[0].numpy(), gx.numpy(), rtol=0, atol=1e-13)


def test_inside_a_mixture():
    mix = [{"weight": 0.5, "chain": [TW, NOISE]}, {"weight": 0.3, "chain": [{"kind": "reverberation", "rt60": 0.1}]}]
    x = torch.stack([unit_clip(b, 7936) for b in range(6)])
    seeds = list(range(20, 26))
    weights = LA.mixture_weights(LA.parse_mixture(mix))
    seen = set()
    for step in range(6):
        z = LA.apply_mixture(x, mix, seeds, step)
        for b, sd in enumerate(seeds):
            c = LA.mixture_choice(sd, step, weights)
            seen.add(c)
            want = x[b] if c < 0 else LA.apply_chain(x[b][None], mix[c]["chain"], [sd], step)[0]
            np.testing.assert_array_equal(z[b].numpy(), want.numpy())
    assert seen == {-1, 0, 1}


# ---- 3. the parser, in Python and in C ----------------------------------------------------------------------------------------------
BAD = [
    ({"kind": "time_warp"}, "depth is required"),
    ({"kind": "time_warp", "period": 0.1}, "depth is required"),
    ({"kind": "time_warp", "depth": 0.04, "seconds": 0.5}, "unknown key"),
    ({"kind": "time_warp", "depth": 0.04, "cents": 60.0}, "unknown key"),
    ({"kind": "time_warp", "depth": "deep"}, "not a number"),
    ({"kind": "time_warp", "depth": float("nan")}, "0 < depth <= 0.1"),
    ({"kind": "time_warp", "depth": float("inf")}, "0 < depth <= 0.1"),
    ({"kind": "time_warp", "depth": 0.0}, "0 < depth <= 0.1"),
    ({"kind": "time_warp", "depth": -0.01}, "0 < depth <= 0.1"),
    ({"kind": "time_warp", "depth": 0.1001}, "0 < depth <= 0.1"),
    ({"kind": "time_warp", "depth": 1e-5}, "rate offset of 0 / 65536"),                    # below 1 / 65536
    ({"kind": "time_warp", "depth": 0.04, "period": float("nan")}, "finite"),
    ({"kind": "time_warp", "depth": 0.04, "period": [0.1, float("inf")]}, "finite"),
    ({"kind": "time_warp", "depth": 0.04, "period": [0.5, 0.1]}, "lo <= hi"),
    ({"kind": "time_warp", "depth": 0.04, "period": 0.0}, "0 < lo"),
    ({"kind": "time_warp", "depth": 0.04, "period": -0.1}, "0 < lo"),
    ({"kind": "time_warp", "depth": 0.04, "period": [0.1, 0.2, 0.3]}, "neither a number"),
    ({"kind": "time_warp", "depth": 0.04, "period": [0.1]}, "neither a number"),
    ({"kind": "time_warp", "depth": 0.04, "period": "slow"}, "neither a number"),
    ({"kind": "time_warp", "depth": 0.04, "period": 0.005}, "no power of two"),            # 80 samples: 2^6
    ({"kind": "time_warp", "depth": 0.04, "period": [0.001, 0.1]}, "no power of two"),      # 16 samples: 2^4
    ({"kind": "time_warp", "depth": 0.04, "period": [0.04, 0.06]}, "no power of two"),      # 640..960: none between
    ({"kind": "time_warp", "depth": 0.04, "period": 100.0}, "no power of two"),            # 1.6e6 samples: 2^21
    ({"kind": "time_warp", "depth": 0.04, "period": [0.1, 200.0]}, "no power of two"),
    ({"kind": "time_warp", "depth": 0.04, "prob": 1.5}, "prob"),
]


@pytest.mark.parametrize("entry,msg", BAD)
def test_parse_chain_refuses(entry, msg):
    with pytest.raises(ValueError, match=msg) as err:
        LA.parse_chain([NOISE, entry])
    assert "loop_attacks[1]" in str(err.value)


def test_parse_chain_accepts_and_keeps_the_tables():
    assert LA.KINDS["time_warp"] == 11 and LA.SPLITTING[8:] == ("time_warp",) and LA.kind_id("time_warp") == 11
    assert (LA.MIN_WARP_EXP, LA.MAX_WARP_EXP, LA.MAX_WARP_DEPTH) == (8, 20, 6553)
    table = _golden("loop_chain_messages.json")
    assert list(LA.KINDS)[:8] == list(table["entries"]) and list(LA.KINDS.values()) == list(range(len(LA.KINDS)))
    assert LA.KINDS["gain_envelope"] == 8 and "gain_envelope" not in LA.SPLITTING and LA.KINDS["band_filter"] == 9 and LA.KINDS["excerpt"] == 10
    assert LA.SPLITTING[6:8] == ("band_filter", "excerpt")
    assert LA.SPLITTING[:6] == ("reverberation", "speed_change", "time_stretch", "pitch_shift", "phase_vocoder", "delete_samples")
    p = LA.parse_chain([{"kind": "time_warp", "depth": 0.04, "period": (0.032, 0.512), "prob": 0.75}])
    assert p == [{"kind": "time_warp", "prob": 0.75, "period": [0.032, 0.512], "depth": 0.04}] and LA.parse_chain(p) == p
    assert LA.parse_chain([{"kind": "time_warp", "depth": 0.04}]) == [{"kind": "time_warp", "prob": 1.0, "period": [0.032, 0.512], "depth": 0.04}]
    assert LA.device_entries_ex(p, 16000) == [(11, 0.75, [9.0, 13.0, 2621.0, 0.0])]
    assert LA.warp_range(LA.parse_chain([{"kind": "time_warp", "depth": 0.1, "period": [0.016, 65.536]}])[0], 16000) == (8, 20, 6553)
    assert LA.warp_range(LA.parse_chain([{"kind": "time_warp", "depth": 1.0 / 65536}])[0], 16000)[2] == 1
    LA.parse_chain([{"kind": "time_warp", "depth": 0.04, "period": 0.01}], sample_rate=48000)      # the rule reads the sample rate
    with pytest.raises(ValueError, match="no power of two"):
        LA.parse_chain([{"kind": "time_warp", "depth": 0.04, "period": 0.02}], sample_rate=8000)
    LA.check_lengths(p, 16000, [513, 100])                                                  # no rule on the lengths
    # the one-split rule against every other splitting kind, in either order, and against itself
    env = {"kind": "gain_envelope", "period": 0.05}
    for s in [table["entries"][k] for k in LA.SPLITTING[:6]] + [FIL, EXC]:
        for chain in ([TW, s], [s, TW], [TW, NOISE, s], [s, env, TW]):
            with pytest.raises(ValueError, match="not both") as err:
                LA.parse_chain(chain)
            assert "time warp" in str(err.value)
    with pytest.raises(ValueError, match="at most one time warp"):
        LA.parse_chain([TW, NOISE, TW])
    for chain in ([NOISE, TW], [TW, NOISE], [env, TW, env, NOISE], [SUP, TW], [NOISE, SUP, TW, NOISE]):
        assert [a["kind"] for a in LA.parse_chain(chain)] == [a["kind"] for a in chain]
    with pytest.raises(ValueError, match="at most 4"):
        LA.parse_chain([NOISE, NOISE, TW, NOISE, NOISE])
    with pytest.raises(ValueError, match="unknown kind") as err:
        LA.parse_chain([{"kind": "time_warps", "depth": 0.04}])
    assert "time_warp" in str(err.value)
    LA.parse_mixture([{"weight": 0.5, "chain": AWARE_CHAIN}, {"weight": 0.5, "chain": [table["entries"]["reverberation"]]}])
    with pytest.raises(ValueError, match=r"loop_attack_mixture\[1\]"):
        LA.parse_mixture([{"weight": 0.5, "chain": [NOISE]}, {"weight": 0.5, "chain": [TW, TW]}])
    from aware_amd.embedding import AWAREEmbedder
    assert AWAREEmbedder(loss="push_extremes", verbose=False, loop_attacks=[SUP, TW, NOISE]).loop_attacks == LA.parse_chain([SUP, TW, NOISE])
    with pytest.raises(ValueError):
        AWAREEmbedder(loss="push_extremes", verbose=False, loop_attacks=[TW, FIL])


def _align(v):
    return (v + 255) & ~255


def test_c_parser_on_the_cpu():
    """csrc/loop_chain.hpp through tests/host_sim/loop_chain_check (built without HIP): rc 0 exactly where parse_chain accepts,
    -1 for each bad parameter, for a fifth entry, beside every other splitting kind and through the older entry point; the byte
    count of a chain with the kind is that of the same chain with a sample deletion in its place plus the two tables, int [B][K]
    and long long [B][K], each at the next 256-byte boundary; a refused pair keeps the count it had before the kind existed; older
    chains keep the bytes recorded in tests/golden/loop_chains_sha256.json."""
    import shutil
    import subprocess
    exe = os.path.join(ROOT, "tests", "host_sim", "loop_chain_check")
    src = os.path.join(ROOT, "tests", "host_sim", "loop_chain_check.cpp")
    hdrs = [os.path.join(ROOT, "aware_amd", "csrc", h) for h in ("loop_chain.hpp", "loop_limits.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [src] + hdrs):
        cxx = ["g++", "-O2", "-std=c++17"] if shutil.which("g++") else ["hipcc", "-O2", "-std=c++17", "-x", "hip", "--offload-host-only"]
        subprocess.run(cxx + ["-o", exe, src], check=True)

    def run(text):
        out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.split()
        return list(zip(map(int, out[0::2]), map(int, out[1::2])))

    spec = importlib.util.spec_from_file_location("loop_attack_bench", os.path.join(ROOT, "tools", "loop_attack_bench.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    fixture = _golden("loop_chains_sha256.json")
    table = _golden("loop_chain_messages.json")
    one = {k: LA.device_entries_ex(LA.parse_chain([a]), 16000)[0] for k, a in table["entries"].items()}
    WC = LA.device_entries_ex(LA.parse_chain(AWARE_CHAIN), 16000)[0]
    assert WC == (11, 0.75, [9.0, 13.0, 2621.0, 0.0])
    BF, XC = (9, 0.75, [15.0, 2458.0, 15565.0, 1638.0]), (10, 0.75, [3000.0, 10000.0, 0.0, 0.0])
    EV, NO, DS = (8, 0.75, [800.0, 8000.0, 0.25]), one["gaussian_noise"], (7, 0.75, [16.0, 512.0, 1.0])
    for ws in fixture["workspace"]:
        dims = _dims_case(ws["dims"])
        B, longest = ws["dims"]["B"], max(ws["dims"]["out_len"])
        with_tables = lambda nbytes, e_lo: _align(_align(nbytes) + 4 * B * LA.warp_breakpoints(longest, e_lo)) + 8 * B * LA.warp_breakpoints(longest, e_lo)
        # accepted: alone, with noise, suppression and envelopes on either side; each with the bytes of its deletion twin and the tables
        chains = [[WC], [NO, WC], [WC, NO], [EV, WC, EV, NO], [one["sample_suppression"], WC, NO], [NO, EV, NO, WC]]
        twins = [[DS if e is WC else e for e in c] for c in chains]
        got = run(dims + "".join(_chain_case(c) for c in chains) + "".join(_chain_case(c) for c in twins))
        for c, (rc, nbytes), (rc2, nbytes2) in zip(chains, got[:len(chains)], got[len(chains):]):
            assert rc == 0 and rc2 == 0 and nbytes == with_tables(nbytes2, 9) > nbytes2 > 0, (c, rc, nbytes, nbytes2)
        # the tables are sized from e_lo
        for e_lo in (8, 14, 20):
            (rc, nbytes), (_, twin) = run(dims + _chain_case([(11, 1.0, [float(e_lo), 20.0, 1.0, 0.0])]) + _chain_case([DS]))
            assert rc == 0 and nbytes == with_tables(twin, e_lo), e_lo
        # ... and inside a mixture, behind a reverberation chain: the choices follow the tables
        m = run(dims + _mixture_case([([one["reverberation"]], 0.5), ([WC, NO], 0.5)])
                + _mixture_case([([one["reverberation"]], 0.5), ([DS, NO], 0.5)]))
        assert m[0][0] == 0 and m[1][0] == 0 and m[0][1] == _align(with_tables(m[1][1] - 4 * B, 9)) + 4 * B
        # the parameters at their limits
        ok = [(11, 1.0, [8.0, 8.0, 1.0, 0.0]), (11, 0.0, [8.0, 20.0, 6553.0, 0.0]), (11, 1.0, [20.0, 20.0, 6553.0, 0.0])]
        assert [rc for rc, _ in run(dims + "".join(_chain_case([e]) for e in ok))] == [0, 0, 0]
        # refused: every bad parameter, a fifth entry, the older entry point
        nan, inf = float("nan"), float("inf")
        bad = [(11, 1.0, [7.0, 13.0, 2621.0, 0.0]), (11, 1.0, [0.0, 13.0, 2621.0, 0.0]), (11, 1.0, [-9.0, 13.0, 2621.0, 0.0]),
               (11, 1.0, [9.5, 13.0, 2621.0, 0.0]), (11, 1.0, [9.0, 13.5, 2621.0, 0.0]), (11, 1.0, [13.0, 9.0, 2621.0, 0.0]),
               (11, 1.0, [9.0, 21.0, 2621.0, 0.0]), (11, 1.0, [9.0, 13.0, 0.0, 0.0]), (11, 1.0, [9.0, 13.0, -1.0, 0.0]),
               (11, 1.0, [9.0, 13.0, 6554.0, 0.0]), (11, 1.0, [9.0, 13.0, 2621.5, 0.0]), (11, 1.0, [9.0, 13.0, 2621.0, 1.0]),
               (11, 1.0, [9.0, 13.0, 2621.0, 0.5]), (11, 1.0, [nan, 13.0, 2621.0, 0.0]), (11, 1.0, [9.0, nan, 2621.0, 0.0]),
               (11, 1.0, [9.0, inf, 2621.0, 0.0]), (11, 1.0, [9.0, 13.0, nan, 0.0]), (11, 1.0, [9.0, 13.0, inf, 0.0]),
               (11, 1.0, [9.0, 13.0, 2621.0, nan]), (11, 1.5, WC[2]), (11, -0.1, WC[2]), (11, nan, WC[2]), (11, 1.0, BF[2]),
               (11, 1.0, XC[2]), (11, 1.0, [0.0]), (12, 1.0, WC[2]), (-1, 1.0, WC[2])]
        assert [rc for rc, _ in run(dims + "".join(_chain_case([e]) for e in bad))] == [-1] * len(bad)
        assert run(dims + _chain_case([NO, NO, WC, NO, NO]))[0] == (-1, 0)
        assert [rc for rc, _ in run(dims + _chain_case([WC], ex=0) + _chain_case([NO, WC], ex=0))] == [-1, -1]
        # beside every other splitting kind, in either order and with an element-wise entry between them: refused, and sized as
        # the chain was sized before the kind existed (the other kind decides)
        for other in [one[k] for k in LA.SPLITTING[:6]] + [BF, XC]:
            got = run(dims + "".join(_chain_case(c) for c in ([WC, other], [other, WC], [other, EV, WC], [other])))
            assert [rc for rc, _ in got[:3]] == [-1, -1, -1], other
            assert got[0][1] == got[1][1] == got[3][1] > 0, other
        got = run(dims + _chain_case([WC, NO, WC]) + _chain_case([WC, NO, NO]))
        assert got[0][0] == -1 and got[1][0] == 0 and got[0][1] == got[1][1]
        # rc 0 exactly where parse_chain accepts: every ordered pair with the kinds of the message table
        for k, a in table["entries"].items():
            for chain, ent in (([TW, a], [WC, one[k]]), ([a, TW], [one[k], WC])):
                try:
                    LA.parse_chain(chain)
                    want = 0
                except ValueError:
                    want = -1
                assert run(dims + _chain_case(ent))[0][0] == want, chain
        # older chains carve what they carved
        text, names = dims, [n for n in ws["bytes"] if n in tool.VARIANTS]
        assert len(names) >= 10
        for name in names:
            text += _chain_case(LA.device_entries_ex(LA.parse_chain(tool.VARIANTS[name]), 16000))
        for name, (rc, nbytes) in zip(names, run(text)):
            assert rc == 0 and nbytes == ws["bytes"][name], (name, rc, nbytes)


# ---- 4. the surface -----------------------------------------------------------------------------------------------------------------
def test_card_keys_reach_the_embedder(tmp_path):
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        text = f.read()
    card = yaml.safe_load(text)
    assert "loop_attacks" not in card and "loop_attack_mixture" not in card              # the committed card keeps its behaviour
    line = "# loop_attacks: [{kind: time_warp, depth: 0.04, period: [0.032, 0.512], prob: 0.75}]"
    assert line in text
    assert LA.parse_chain(yaml.safe_load(line[2:])["loop_attacks"]) == LA.parse_chain(AWARE_CHAIN)
    card["loop_attacks"] = yaml.safe_load(line[2:])["loop_attacks"] + [{"kind": "gaussian_noise", "snr_db": 20.0}]
    card["loop_attack_seed"] = 5
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.loop_attacks == [{"kind": "time_warp", "prob": 0.75, "period": [0.032, 0.512], "depth": 0.04},
                                {"kind": "gaussian_noise", "prob": 1.0, "snr_db": 20.0}]
    assert emb.loop_attack_seed == 5
    del card["loop_attacks"]
    card["loop_attack_mixture"] = [{"weight": 0.5, "chain": [{"kind": "time_warp", "depth": 0.02, "period": 0.064}]},
                                   {"weight": 0.5, "chain": [{"kind": "sample_suppression", "seconds": 0.3}]}]
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.loop_attack_mixture[0] == {"weight": 0.5, "chain": [{"kind": "time_warp", "prob": 1.0, "period": 0.064, "depth": 0.02}]}
    del card["loop_attack_mixture"]
    card["loop_attacks"] = [{"kind": "time_warp", "depth": 0.5}]
    p.write_text(yaml.safe_dump(card))
    assert load(str(p)) is None                               # a stage that fails is reported as None, as everywhere in load()
    from aware_amd.embedding import AWAREEmbedder
    with pytest.raises(NotImplementedError, match="loop_attacks"):                          # the kind is for the card route
        AWAREEmbedder(frame_length=512, hop_length=128, win_length=512, general_geometry=True, verbose=False, loss="push_extremes",
                      detection_net_cfg={"n_fft": 512}, loop_attacks=AWARE_CHAIN)


def test_abi_symbols_and_bad_arguments():
    from aware_amd import _lib, attacks as A
    lib = _lib.load_library()
    assert "aware_time_warp" in _lib.SIGNATURES and hasattr(lib, "aware_time_warp")
    assert "loop_warp_kernels.hip" in _lib.SOURCES and len(_lib.SIGNATURES["aware_time_warp"][1]) == 14
    assert lib.aware_version() == 350
    with open(os.path.join(ROOT, "include", "aware_hip.h")) as f:
        hdr = f.read()
    assert "#define AWARE_LOOP_TIME_WARP 11" in hdr and "int aware_time_warp(const float* in, const int* off" in hdr
    with open(os.path.join(ROOT, "aware_amd", "csrc", "loop_limits.hpp")) as f:
        lim = f.read()
    assert "kLoopTimeWarp = 11" in lim and "kWarpMinExp = 8, kWarpMaxExp = 20, kWarpMaxDepth = 6553" in lim
    seeds = (C.c_uint32 * 1)(0)
    ent = (_lib.LoopAttackEx * 1)(_lib.LoopAttackEx(11, 0.75, (C.c_float * 4)(9.0, 13.0, 2621.0, 0.0)))
    assert lib.aware_embed_set_loop_attacks_ex(None, ent, 1, seeds, None, 0, None) == -1          # no handle
    assert lib.aware_embed_loop_attack_workspace_bytes_ex(None, ent, 1) == 0
    old = (_lib.LoopAttack * 1)(_lib.LoopAttack(11, 9.0, 1.0))
    assert lib.aware_embed_set_loop_attacks(None, old, 1, seeds, None, 0, None) == -1
    # the stand-alone entry refuses null pointers, sizes out of range and aliasing before anything touches a device
    call = lambda a, B=1, max_len=16000, stride=65, adjoint=0: lib.aware_time_warp(a[0], a[1], a[2], B, max_len, a[3], a[4], a[5], stride,
                                                                                  a[6], a[7], a[8], adjoint, None)
    assert call([None] * 9) == -1
    p, q = C.c_void_p(256), C.c_void_p(512)                  # never dereferenced: every call below is refused
    for i in range(9):                                       # each pointer in turn
        a = [p] * 8 + [q]
        a[i] = None
        assert call(a) == -1, i
    ok = [p] * 8 + [q]
    for kw in (dict(B=0), dict(B=65536), dict(B=-1), dict(max_len=0), dict(max_len=(1 << 30) + 1), dict(stride=2), dict(stride=0),
               dict(stride=-5), dict(adjoint=2), dict(adjoint=-1)):
        assert call(ok, **kw) == -1, kw
    assert call([p] * 9) == -1                                                              # out == in
    assert {"TimeWarp", "Flutter", "SpeedChange"} <= set(A.ATTACKS)
    assert A.make_attack("TimeWarp", depth=0.04).name == "time_warp_0.04"
    assert A.make_attack("Flutter", depth=0.03, hz=6.0, phase=2.0).name == "flutter_0.03_6.0"
    assert A.make_attack("TimeWarp", depth=0.04, period=0.064, seed=3).entry == LA.parse_chain([{"kind": "time_warp", "depth": 0.04, "period": 0.064}])[0]
    assert [type(a).__name__ for a in A.config3_attack_stack()] == ["Resample", "LowPassFilter", "GaussianNoise", "PCMBitDepthConversion"]
    assert len(A.reference_attack_list()) == 13
    for kw in (dict(depth=0.0), dict(depth=0.2), dict(depth=float("nan")), dict(depth=0.04, period=0.001), dict(depth=0.04, period=[0.5, 0.1])):
        with pytest.raises(ValueError):
            A.TimeWarp(**kw)
    for kw in (dict(depth=0.0, hz=1.0), dict(depth=0.1, hz=1.0), dict(depth=0.03, hz=0.0), dict(depth=0.03, hz=float("inf")),
               dict(depth=0.03, hz=1.0, phase=float("nan"))):
        with pytest.raises(ValueError):
            A.Flutter(**kw)
    m = A.Flutter(0.03, 6.0, 2.0).rates(16000, 16000)
    assert len(m) == LA.warp_breakpoints(16000, 8) and m[0] == round(65536 * 0.03 * math.sin(2.0)) and np.abs(m).max() <= 1967


# ---- 5. the value claim, on the CPU -------------------------------------------------------------------------------------------------
FLUTTERS = [(hz, phi) for hz in (0.5, 2.0, 6.0, 12.0) for phi in (0.0, 2.0)]


def flutter(y, depth, hz, phi, sr=16000):
    """y [B, n] played at the speed 1 + depth sin(2 pi hz t + phi): read at the integral of the speed through a cubic spline
    (scipy.interpolate.CubicSpline), zero past the last sample.  Shares no code with the loop's operator."""
    from scipy.interpolate import CubicSpline
    n = y.shape[-1]
    i = np.arange(n, dtype=np.float64)
    pos = i + depth * sr / (2.0 * np.pi * hz) * (np.cos(phi) - np.cos(2.0 * np.pi * hz * i / sr + phi))
    inside = (pos >= 0.0) & (pos <= n - 1.0)
    out = CubicSpline(i, np.asarray(y, dtype=np.float64), axis=-1)(np.clip(pos, 0.0, n - 1.0))
    return np.where(inside, out, 0.0).astype(np.float32)


def flutter_table(read, y, depth):
    """{(hz, phi): BER %} of the eight flutters at this depth; read(z) is the BER of a batch."""
    return {k: read(flutter(y, depth, *k)) for k in FLUTTERS}


def report(names, tables, clean, snr, depth):
    for k in FLUTTERS:
        print(f"depth {depth}, {k[0]:4.1f} Hz, phase {k[1]:.1f}: " + "   ".join(f"{n} {t[k]:6.2f} %" for n, t in zip(names, tables)))
    means = [float(np.mean(list(t.values()))) for t in tables]
    print(f"depth {depth}: means " + " / ".join(f"{n} {m:.2f} %" for n, m in zip(names, means)) + "; clean "
          + " / ".join(f"{c:.2f} %" for c in clean) + "; SNR against the host " + " / ".join(f"{s:.1f} dB" for s in snr))
    return means


def test_warp_in_the_loop_survives_wow_and_flutter(value_setup):
    """Four 1 s clips, 400 steps, seeds 0..3: BER under eight sinusoidal flutters the loop's model does not contain (speed
    1 + 0.03 sin(2 pi hz t + phi), hz 0.5 / 2 / 6 / 12, phi 0 / 2.0, through scipy's cubic spline) of the plain embedding, of the
    embedding with speed_change(cents 60, prob 0.75) and of the embedding with time_warp(depth 0.04, period 0.032-0.512 s, prob
    0.75) inside the loop.  Clean 0 % for all three, the plain mean at least 10 %, the warp-aware mean at most half of it and
    below the speed-aware mean.  Measured with this restatement at depth 0.03, per rate as phi 0 / 2.0: plain 42.5 / 30, 36.25 / 25,
    43.75 / 43.75, 41.25 / 52.5 %, mean 39.38 %; speed-aware 0 / 8.75, 11.25 / 11.25, 23.75 / 22.5, 23.75 / 25 %, mean 15.78 %;
    warp-aware 0 / 1.25, 1.25 / 0, 3.75 / 2.5, 8.75 / 13.75 %, mean 3.91 %; clean 0 % for all; SNR 15.8 / 15.0 / 15.0 dB.  The row
    at depth 0.01 is reported too: every cell is 0 % for all three, the plain watermark already survives it (DESIGN.md section
    35)."""
    plain, audio, bits, wm, y0 = value_setup
    ys = [y0] + [AttackedEmbedder(c, [0, 1, 2, 3]).embed(audio, wm)[0].numpy() for c in (SPEED_CHAIN, AWARE_CHAIN)]
    names = ["plain", "speed-aware", "warp-aware"]
    read = lambda z: ber(plain, bits, z)
    clean, snr = [read(y) for y in ys], [snr_db(audio, y) for y in ys]
    report(names, [flutter_table(read, y, 0.01) for y in ys], clean, snr, 0.01)
    m0, m1, m2 = report(names, [flutter_table(read, y, 0.03) for y in ys], clean, snr, 0.03)
    assert clean == [0.0, 0.0, 0.0]
    assert m0 >= 10.0
    assert m2 <= 0.5 * m0
    assert m2 < m1
