"""Frequency shifts inside the embed loop (EXTENSION, chain kind 12): the torch restatement of aware_amd/embedding/loop_attacks.py
against a plain loop over the definition, its adjoint, the FFT analytic-signal shift as the independent model, its draw and its
place in a chain, the parser in Python and in C (csrc/loop_chain.hpp through tests/host_sim/loop_chain_check on the CPU), the card
keys, the ABI, and the value claim on the CPU: what a frequency shift in the loop buys under single-sideband shifts made with
scipy.signal.hilbert, through the oracle's embed loop.  No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, make_clip  # noqa: F401
from aware_amd.embedding import loop_attacks as LA
from test_loop_attacks_host import AttackedEmbedder, _chain_case, _dims_case, _golden, _mixture_case, ber, loop_chain_check, value_setup  # noqa: F401
from test_loop_gain_host import snr_db

AWARE_CHAIN = [{"kind": "frequency_shift", "hz": 120.0, "prob": 0.75}]
SHIFT = {"kind": "frequency_shift", "hz": 120.0}
NOISE = {"kind": "gaussian_noise", "snr_db": 10.0}
ONE = 1 << 20
SHIFTS = [0, 1, -7864, 65536, -65536]                         # d, in units of sr / 2^20 Hz
PHASES = [0, 1 << 19, ONE - 1]                               # p0, in units of 2^-20 turn
SUM_H = 3.4103                                               # sum |h| of the 255 Hilbert taps
CLAIM_HZ = [-100.0, -50.0, -20.0, -10.0, 10.0, 20.0, 50.0, 100.0]


# ---- 1. the model -------------------------------------------------------------------------------------------------------------------
def plain_taps():
    """h[k], k = -127..127, tap by tap from the issue's definition."""
    out = []
    for k in range(-127, 128):
        if k % 2 == 0:
            out.append(0.0)
            continue
        out.append((0.54 + 0.46 * math.cos(math.pi * k / 127)) * 2.0 / (math.pi * k))
    return out


def plain_hilbert(x, i, h):
    """(Hx)[i] = sum_k h[k] x[i - k], x zero outside the clip."""
    n = len(x)
    return math.fsum(h[k + 127] * x[i - k] for k in range(-127, 128) if 0 <= i - k < n)


def plain_phase(i, d, p0):
    return 2.0 * math.pi * ((p0 + i * d) % ONE) / ONE


def test_taps_are_the_definition():
    want = np.array(plain_taps())
    h64 = LA.hilbert_taps()
    assert h64.dtype == np.float64 and h64.shape == (255,)
    np.testing.assert_allclose(h64, want, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(h64, -h64[::-1])                                # antisymmetric: H^T = -H
    assert np.all(h64[np.arange(-127, 128) % 2 == 0] == 0.0) and h64[127] == 0.0  # even taps, zero included, exactly 0
    assert np.all(h64[128::2] > 0.0)                                              # the odd taps of positive k
    assert abs(float(np.abs(h64).sum()) - SUM_H) <= 1e-4
    h32 = LA.hilbert_taps(np.float32)
    assert h32.dtype == np.float32 and h32.shape == (255,)
    assert np.abs(h32.astype(np.float64) - want).max() <= 1e-6
    assert np.all(h32[np.arange(-127, 128) % 2 == 0] == 0.0)


@pytest.mark.parametrize("n", [100, 254, 255, 4099])
def test_frequency_shift_is_the_definition(n):
    """Two lengths shorter than the taps, one of exactly their count, one of several tiles of any kernel (at a stride and at both
    ends), every d and p0 of the issue."""
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n)
    h = plain_taps()
    step = 1 if n < 1000 else 97
    idx = sorted(i for i in set(range(0, n, step)) | set(range(130)) | set(range(n - 130, n)) if 0 <= i < n)
    hx = {i: plain_hilbert(list(x), i, h) for i in idx}
    xt = torch.from_numpy(x)
    for d in SHIFTS:
        for p0 in PHASES:
            z = LA.frequency_shift(xt, d, p0).numpy()
            for i in idx:
                phi = plain_phase(i, d, p0)
                assert abs(z[i] - (x[i] * math.cos(phi) - hx[i] * math.sin(phi))) <= 1e-12, (n, d, p0, i)
    np.testing.assert_array_equal(LA.frequency_shift(xt, 0, 0).numpy(), x)         # phi = 0: cos 1, sin 0
    z32 = LA.frequency_shift(xt.float(), -7864, 5)
    assert z32.dtype == torch.float32 and z32.shape == (n,)
    rag = LA.frequency_shift([xt, xt[:50]], [-7864, 65536], [0, ONE - 1])
    assert [r.shape[0] for r in rag] == [n, 50]
    np.testing.assert_array_equal(rag[0].numpy(), LA.frequency_shift(xt, -7864, 0).numpy())
    np.testing.assert_array_equal(rag[1].numpy(), LA.frequency_shift(xt[:50], 65536, ONE - 1).numpy())
    for bad in ((65537, 0), (-65537, 0), (1, -1), (1, ONE)):
        with pytest.raises(ValueError):
            LA.frequency_shift(xt, *bad)


@pytest.mark.parametrize("d,p0", [(3277, 0), (-7864, 1 << 19), (65536, ONE - 1), (1, 12345)])
def test_the_adjoint(d, p0):
    rng = np.random.default_rng(7 + abs(d))
    for n in (100, 300, 4099):
        x, w = torch.from_numpy(rng.standard_normal(n)), torch.from_numpy(rng.standard_normal(n))
        lhs = float(torch.dot(LA.frequency_shift(x, d, p0), w))
        rhs = float(torch.dot(x, LA.frequency_shift_adjoint(w, d, p0)))
        assert abs(lhs - rhs) <= 1e-12 * (1.0 + abs(lhs)), (n, lhs, rhs)
        # ... and autograd agrees with the stated adjoint
        xg = x.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(torch.dot(LA.frequency_shift(xg, d, p0), w), xg)
        assert float((g - LA.frequency_shift_adjoint(w, d, p0)).abs().max()) <= 1e-12
    x = torch.from_numpy(rng.standard_normal(300)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: LA.frequency_shift(v, d, p0), (x,), eps=1e-6, atol=1e-7)
    rag = LA.frequency_shift_adjoint([x.detach(), x.detach()[:50]], [d, -d], [p0, 0])
    assert [r.shape[0] for r in rag] == [300, 50]


@pytest.mark.parametrize("hz", [50.0, -120.0])
def test_against_the_fft_analytic_signal_shift(hz):
    """The independent model: a 1 s Gaussian signal band-passed to 150-7000 Hz, shifted as Re(hilbert(x) e^{j 2 pi (d / 2^20) i}).
    Relative L2 over [512, n - 512) at most 1e-3 (measured 4.1e-4 at both).  Also fixes the sign: a positive d shifts upwards."""
    from scipy.signal import hilbert
    n, sr = 16000, 16000
    spec = np.fft.rfft(np.random.default_rng(5).standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / sr)
    spec[(f < 150.0) | (f > 7000.0)] = 0.0
    x = np.fft.irfft(spec, n)
    d = LA.shift_increment(hz, sr)
    assert d == {50.0: 3277, -120.0: -7864}[hz]
    want = np.real(hilbert(x) * np.exp(2j * np.pi * (d / ONE) * np.arange(n)))
    z = LA.frequency_shift(torch.from_numpy(x), d, 0).numpy()
    sl = slice(512, n - 512)
    rel = float(np.linalg.norm(z[sl] - want[sl]) / np.linalg.norm(want[sl]))
    print(f"{hz:+.0f} Hz (d = {d}): relative L2 against the FFT analytic-signal shift over the interior = {rel:.2e}")
    assert rel <= 1e-3
    # the spectral centroid moves by the shift, in its direction
    cen = lambda v: float((f * np.abs(np.fft.rfft(v)) ** 2).sum() / (np.abs(np.fft.rfft(v)) ** 2).sum())
    assert abs((cen(z) - cen(x)) - hz) < 5.0


# ---- 2. the draw and the chain ------------------------------------------------------------------------------------------------------
def test_draws_stay_in_range_and_differ():
    chain = LA.parse_chain(AWARE_CHAIN)
    assert chain == [{"kind": "frequency_shift", "prob": 0.75, "hz": [-120.0, 120.0]}]
    d_lo, d_hi = LA.shift_range(chain[0], 16000)
    assert (d_lo, d_hi) == (-7864, 7864)
    draws = []
    for step in range(300):
        r = LA.entry_draw(3, step, 0)
        d, p0 = LA.shift_draw(chain[0], r, 16000)
        assert d_lo <= d <= d_hi and 0 <= p0 < ONE
        # the definition, in Python integers
        assert d == d_lo + ((int(r[1]) * (d_hi - d_lo + 1)) >> 32) and p0 == int(r[2]) >> 12
        draws.append((d, p0))
    ds, ps = np.array([d for d, _ in draws]), np.array([p for _, p in draws])
    assert len(set(draws)) > 290
    # the spread of 300 uniform draws: both halves and both ends of the range, a mean near its centre
    assert ds.min() < d_lo + 400 and ds.max() > d_hi - 400 and abs(ds.mean()) < 4 * (d_hi - d_lo) / math.sqrt(12 * 300)
    assert (ds < 0).sum() > 110 and (ds > 0).sum() > 110
    assert ps.min() < ONE // 16 and ps.max() > ONE - ONE // 16 and abs(ps.mean() - ONE / 2) < 4 * ONE / math.sqrt(12 * 300)
    # a scalar hz and the pair it means agree; a pair is taken as written
    pair = LA.parse_chain([dict(AWARE_CHAIN[0], hz=[-120.0, 120.0])])[0]
    assert pair == chain[0]
    one_sided = LA.parse_chain([{"kind": "frequency_shift", "hz": [20.0, 120.0]}])[0]
    assert LA.shift_range(one_sided, 16000) == (1311, 7864)
    for step in range(50):
        r = LA.entry_draw(1, step, 0)
        assert LA.shift_draw(pair, r, 16000) == LA.shift_draw(chain[0], r, 16000)
        assert 1311 <= LA.shift_draw(one_sided, r, 16000)[0] <= 7864
    fixed = LA.parse_chain([{"kind": "frequency_shift", "hz": [50.0, 50.0]}])[0]
    assert {LA.shift_draw(fixed, LA.entry_draw(1, s, 0), 16000)[0] for s in range(20)} == {3277}
    # across step, clip and entry index
    base = LA.shift_draw(chain[0], LA.entry_draw(3, 5, 0), 16000)
    assert base != LA.shift_draw(chain[0], LA.entry_draw(3, 6, 0), 16000)
    assert base != LA.shift_draw(chain[0], LA.entry_draw(4, 5, 0), 16000)
    assert base != LA.shift_draw(chain[0], LA.entry_draw(3, 5, 1), 16000)


def test_prob_and_order_in_a_chain():
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((1, 2000)))
    for prob, want in ((0.0, 0), (1.0, 400)):
        ch = [dict(AWARE_CHAIN[0], prob=prob)]
        fired = sum(not torch.equal(LA.apply_chain(x, ch, [9], s), x) for s in range(400))
        assert fired == want
    fired = sum(LA.fires(LA.entry_draw(9, s, 0)[0], 0.75) for s in range(400))
    assert abs(fired - 300) <= 3 * math.sqrt(400 * 0.75 * 0.25)
    got = sum(not torch.equal(LA.apply_chain(x, AWARE_CHAIN, [9], s), x) for s in range(400))
    assert got == fired
    # the chain's output is the drawn shift of the clip; a clip that does not fire is a copy, bit for bit
    entry = LA.parse_chain(AWARE_CHAIN)[0]
    for s in range(8):
        r = LA.entry_draw(9, s, 0)
        z = LA.apply_chain(x, AWARE_CHAIN, [9], s)[0]
        want = LA.frequency_shift(x[0], *LA.shift_draw(entry, r, 16000)) if LA.fires(r[0], 0.75) else x[0]
        assert torch.equal(z, want)
    # noise in front of the shift is shifted with the signal; noise behind it takes its sigma from the shifted signal
    d, p0 = LA.shift_draw(LA.parse_chain([NOISE, SHIFT])[1], LA.entry_draw(9, 2, 1), 16000)
    z = LA.apply_chain(x, [NOISE, SHIFT], [9], 2)[0]
    noisy = LA.apply_chain(x, [NOISE], [9], 2)[0]
    assert torch.equal(z, LA.frequency_shift(noisy, d, p0))
    d, p0 = LA.shift_draw(LA.parse_chain([SHIFT])[0], LA.entry_draw(9, 2, 0), 16000)
    z = LA.apply_chain(x, [SHIFT, NOISE], [9], 2)[0]
    f = LA.frequency_shift(x[0], d, p0)
    sigma = math.sqrt(float(np.mean(f.numpy() ** 2)) / 10.0)
    np.testing.assert_allclose((z - f).numpy(), sigma * LA.normal_draws(2000, 9, 2, 1), rtol=0, atol=1e-12)
    # in a mixture: each clip goes through the chain it draws
    mix = [{"weight": 0.5, "chain": AWARE_CHAIN}, {"weight": 0.5, "chain": [NOISE]}]
    xs = torch.from_numpy(np.random.default_rng(1).standard_normal((6, 600)))
    seeds = list(range(6))
    out = LA.apply_mixture(xs, mix, seeds, 3)
    choice = LA.mixture_choices(seeds, 3, [0.5, 0.5])
    assert set(choice.tolist()) == {0, 1}
    for b in range(6):
        assert torch.equal(out[b], LA.apply_chain(xs[b:b + 1], mix[choice[b]]["chain"], [seeds[b]], 3)[0])


# ---- 3. the parsers -----------------------------------------------------------------------------------------------------------------
BAD = [
    ({"kind": "frequency_shift"}, "hz is required"),
    ({"kind": "frequency_shift", "hz": float("nan")}, "hz"),
    ({"kind": "frequency_shift", "hz": float("inf")}, "finite"),
    ({"kind": "frequency_shift", "hz": [-50.0, float("inf")]}, "finite"),
    ({"kind": "frequency_shift", "hz": [float("nan"), 50.0]}, "finite"),
    ({"kind": "frequency_shift", "hz": [120.0, -120.0]}, "lo <= hi"),
    ({"kind": "frequency_shift", "hz": 0.0}, "> 0"),
    ({"kind": "frequency_shift", "hz": -120.0}, "> 0"),
    ({"kind": "frequency_shift", "hz": [1.0, 2.0, 3.0]}, "neither a number"),
    ({"kind": "frequency_shift", "hz": "wide"}, "neither a number"),
    ({"kind": "frequency_shift", "hz": 1000.1}, "outside"),                                   # d = 65543
    ({"kind": "frequency_shift", "hz": [-1000.1, 0.0]}, "outside"),
    ({"kind": "frequency_shift", "hz": [0.0, 2000.0]}, "outside"),
    ({"kind": "frequency_shift", "hz": 120.0, "phase": 0.5}, "unknown key"),
    ({"kind": "frequency_shift", "hz": 120.0, "prob": 1.5}, "prob"),
    ({"kind": "frequency_shift", "hz": 120.0, "prob": -0.1}, "prob"),
]


@pytest.mark.parametrize("entry,msg", BAD)
def test_parse_chain_refuses(entry, msg):
    with pytest.raises(ValueError, match=msg) as err:
        LA.parse_chain([NOISE, entry])
    assert "loop_attacks[1] (frequency_shift): " in str(err.value)


def test_parse_chain_accepts_and_keeps_the_tables():
    assert LA.KINDS["frequency_shift"] == 12 and LA.kind_id("frequency_shift") == 12
    # a kind with a stage of its own, listed in STAGED: SPLITTING is closed at the time warp (tests/test_loop_warp_host.py)
    assert LA.STAGED == ("frequency_shift",) and LA.SPLITTING[8:] == ("time_warp",) and not LA.TABLE[12].splits
    assert LA.MAX_SHIFT == 65536 and LA.PHASE_ONE == ONE
    table = _golden("loop_kinds_table.json")
    assert list(LA.KINDS)[:12] == list(table["entries"]) and list(LA.KINDS.values()) == list(range(13))
    # the device tuples, as literals
    p = LA.parse_chain(AWARE_CHAIN)
    assert LA.parse_chain(p) == p
    assert LA.device_entries_ex(p, 16000) == [(12, 0.75, [-7864.0, 7864.0, 0.0, 0.0])]
    assert LA.device_entries_ex(LA.parse_chain(AWARE_CHAIN, 44100), 44100) == [(12, 0.75, [-2853.0, 2853.0, 0.0, 0.0])]
    assert LA.device_entries_ex(LA.parse_chain([{"kind": "frequency_shift", "hz": [-50.0, 120.0]}]), 16000) == [(12, 1.0, [-3277.0, 7864.0, 0.0, 0.0])]
    assert LA.shift_range(LA.parse_chain([{"kind": "frequency_shift", "hz": 1000.0}])[0], 16000) == (-65536, 65536)     # sr / 16 itself
    LA.parse_chain([{"kind": "frequency_shift", "hz": 2000.0}], sample_rate=48000)              # the rule reads the sample rate
    with pytest.raises(ValueError, match="outside"):
        LA.parse_chain([{"kind": "frequency_shift", "hz": 600.0}], sample_rate=8000)
    LA.check_lengths(p, 16000, [1, 100])                                                        # no rule on the lengths
    # the one-split rule against every other splitting kind, in either order, and against itself
    env = {"kind": "gain_envelope", "period": 0.05}
    for kind in LA.SPLITTING[:9]:
        s = table["entries"][kind]
        for chain in ([SHIFT, s], [s, SHIFT], [SHIFT, NOISE, s], [s, env, SHIFT]):
            with pytest.raises(ValueError, match="not both") as err:
                LA.parse_chain(chain)
            assert "frequency shift" in str(err.value) and f"loop_attacks[{len(chain) - 1}]" in str(err.value)
    with pytest.raises(ValueError, match="at most one frequency shift per chain"):
        LA.parse_chain([SHIFT, NOISE, SHIFT])
    for chain in ([NOISE, SHIFT], [SHIFT, NOISE], [env, SHIFT, env, NOISE], [table["entries"]["sample_suppression"], SHIFT]):
        assert [a["kind"] for a in LA.parse_chain(chain)] == [a["kind"] for a in chain]
    with pytest.raises(ValueError, match="at most 4"):
        LA.parse_chain([NOISE, NOISE, SHIFT, NOISE, NOISE])
    with pytest.raises(ValueError, match="unknown kind"):
        LA.parse_chain([{"kind": "frequency_shifts", "hz": 120.0}])
    LA.parse_mixture([{"weight": 0.5, "chain": AWARE_CHAIN}, {"weight": 0.5, "chain": [table["entries"]["reverberation"]]}])
    with pytest.raises(ValueError, match=r"loop_attack_mixture\[1\]"):
        LA.parse_mixture([{"weight": 0.5, "chain": [NOISE]}, {"weight": 0.5, "chain": [SHIFT, SHIFT]}])
    from aware_amd.embedding import AWAREEmbedder
    sup = table["entries"]["sample_suppression"]
    assert AWAREEmbedder(loss="push_extremes", verbose=False, loop_attacks=[sup, SHIFT, NOISE]).loop_attacks == LA.parse_chain([sup, SHIFT, NOISE])
    with pytest.raises(ValueError):
        AWAREEmbedder(loss="push_extremes", verbose=False, loop_attacks=[SHIFT, table["entries"]["band_filter"]])


def test_c_parser_on_the_cpu():
    """csrc/loop_chain.hpp through tests/host_sim/loop_chain_check (built without HIP): rc 0 exactly where parse_chain accepts,
    -1 for each bad parameter (the time warp's [9, 13, 2621, 0] included), for a fifth entry, beside every other splitting kind in
    either order and through the older entry point; the byte count of a chain with the kind is that of the same chain with a
    sample deletion in its place, alone and inside a mixture; older chains keep their bytes."""
    run = loop_chain_check()
    fixture = _golden("loop_chains_sha256.json")
    table = _golden("loop_kinds_table.json")
    one = {k: LA.device_entries_ex(LA.parse_chain([a]), 16000)[0] for k, a in table["entries"].items()}
    FS = LA.device_entries_ex(LA.parse_chain(AWARE_CHAIN), 16000)[0]
    assert FS == (12, 0.75, [-7864.0, 7864.0, 0.0, 0.0])
    EV, NO, DS = (8, 0.75, [800.0, 8000.0, 0.25]), one["gaussian_noise"], (7, 0.75, [16.0, 512.0, 1.0])
    for ws in fixture["workspace"]:
        dims = _dims_case(ws["dims"])
        # accepted: alone, with noise, suppression and envelopes on either side; each with the bytes of its deletion twin
        chains = [[FS], [NO, FS], [FS, NO], [EV, FS, EV, NO], [one["sample_suppression"], FS, NO], [NO, EV, NO, FS]]
        twins = [[DS if e is FS else e for e in c] for c in chains]
        got = run(dims + "".join(_chain_case(c) for c in chains) + "".join(_chain_case(c) for c in twins))
        for c, (rc, nbytes), (rc2, nbytes2) in zip(chains, got[:len(chains)], got[len(chains):]):
            assert rc == 0 and rc2 == 0 and nbytes == nbytes2 > 0, (c, rc, nbytes, nbytes2)
        # ... and inside a mixture, behind a reverberation chain
        m = run(dims + _mixture_case([([one["reverberation"]], 0.5), ([FS, NO], 0.5)])
                + _mixture_case([([one["reverberation"]], 0.5), ([DS, NO], 0.5)]))
        assert m[0][0] == 0 and m[1][0] == 0 and m[0][1] == m[1][1] > 0
        # the parameters at their limits
        ok = [(12, 1.0, [-65536.0, 65536.0, 0.0, 0.0]), (12, 0.0, [0.0, 0.0, 0.0, 0.0]), (12, 1.0, [65536.0, 65536.0, 0.0, 0.0]),
              (12, 1.0, [-65536.0, -65536.0, 0.0, 0.0]), (12, 1.0, [-1.0, 1.0, 0.0, 0.0])]
        assert [rc for rc, _ in run(dims + "".join(_chain_case([e]) for e in ok))] == [0] * len(ok)
        # refused: every bad parameter, a fifth entry, the older entry point
        nan, inf = float("nan"), float("inf")
        bad = [(12, 1.0, [-65537.0, 7864.0, 0.0, 0.0]), (12, 1.0, [-7864.0, 65537.0, 0.0, 0.0]), (12, 1.0, [7864.0, -7864.0, 0.0, 0.0]),
               (12, 1.0, [-7864.5, 7864.0, 0.0, 0.0]), (12, 1.0, [-7864.0, 7864.5, 0.0, 0.0]), (12, 1.0, [nan, 7864.0, 0.0, 0.0]),
               (12, 1.0, [-7864.0, nan, 0.0, 0.0]), (12, 1.0, [-inf, 7864.0, 0.0, 0.0]), (12, 1.0, [-7864.0, inf, 0.0, 0.0]),
               (12, 1.0, [-7864.0, 7864.0, 1.0, 0.0]), (12, 1.0, [-7864.0, 7864.0, 0.0, 1.0]), (12, 1.0, [-7864.0, 7864.0, nan, 0.0]),
               (12, 1.0, [-7864.0, 7864.0, 0.0, nan]), (12, 1.0, [9.0, 13.0, 2621.0, 0.0]), (12, 1.5, FS[2]), (12, nan, FS[2]),
               (12, -0.1, FS[2]), (13, 1.0, FS[2])]
        assert [rc for rc, _ in run(dims + "".join(_chain_case([e]) for e in bad))] == [-1] * len(bad)
        assert run(dims + _chain_case([NO, NO, FS, NO, NO]))[0] == (-1, 0)
        assert [rc for rc, _ in run(dims + _chain_case([FS], ex=0) + _chain_case([NO, FS], ex=0))] == [-1, -1]
        # beside every other splitting kind, in either order and with an element-wise entry between them, and beside itself:
        # refused, and sized as the chain was sized before the kind existed (the other kind decides)
        for k in LA.SPLITTING[:9]:
            got = run(dims + "".join(_chain_case(c) for c in ([FS, one[k]], [one[k], FS], [one[k], EV, FS], [one[k]])))
            assert [rc for rc, _ in got[:3]] == [-1, -1, -1], k
            # (a refused time warp's tables are sized from whatever range the parser last read: only the chains that parse
            # the warp first have the warp's own count)
            assert got[1][1] == got[2][1] == got[3][1] > 0 and (got[0][1] == got[3][1] or k == "time_warp") and got[0][1] > 0, k
        got = run(dims + _chain_case([FS, NO, FS]) + _chain_case([DS, NO, NO]))
        assert got[0][0] == -1 and got[0][1] == got[1][1]
        # rc is 0 exactly where parse_chain accepts
        for names in (["frequency_shift"], ["gaussian_noise", "frequency_shift"], ["frequency_shift", "band_filter"],
                      ["time_warp", "frequency_shift"], ["frequency_shift", "frequency_shift"], ["gain_envelope", "frequency_shift", "gain_envelope"]):
            entries = [SHIFT if k == "frequency_shift" else table["entries"][k] for k in names]
            try:
                LA.parse_chain(entries)
                accepted = True
            except ValueError:
                accepted = False
            dev = [LA.device_entries_ex(LA.parse_chain([e]), 16000)[0] for e in entries]
            assert (run(dims + _chain_case(dev))[0][0] == 0) == accepted, names
        # older chains carve what they carved
        if "noise" in ws["bytes"]:
            assert run(dims + _chain_case([NO]))[0] == (0, ws["bytes"]["noise"])


# ---- 4. the surface -----------------------------------------------------------------------------------------------------------------
def test_card_keys_reach_the_embedder(tmp_path):
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        text = f.read()
    card = yaml.safe_load(text)
    assert "loop_attacks" not in card and "loop_attack_mixture" not in card              # the committed card keeps its behaviour
    line = "# loop_attacks: [{kind: frequency_shift, hz: 120.0, prob: 0.75}]"
    assert line in text
    card["loop_attacks"] = yaml.safe_load(line[2:])["loop_attacks"] + [{"kind": "gaussian_noise", "snr_db": 20.0}]
    card["loop_attack_seed"] = 5
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.loop_attacks == [{"kind": "frequency_shift", "prob": 0.75, "hz": [-120.0, 120.0]},
                                {"kind": "gaussian_noise", "prob": 1.0, "snr_db": 20.0}]
    assert emb.loop_attack_seed == 5
    del card["loop_attacks"]
    card["loop_attack_mixture"] = [{"weight": 0.5, "chain": [{"kind": "frequency_shift", "hz": [20.0, 60.0]}]},
                                   {"weight": 0.5, "chain": [{"kind": "sample_suppression", "seconds": 0.3}]}]
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.loop_attack_mixture[0] == {"weight": 0.5, "chain": [{"kind": "frequency_shift", "prob": 1.0, "hz": [20.0, 60.0]}]}
    del card["loop_attack_mixture"]
    card["loop_attacks"] = [{"kind": "frequency_shift", "hz": 1200.0}]
    p.write_text(yaml.safe_dump(card))
    assert load(str(p)) is None                               # a stage that fails is reported as None, as everywhere in load()
    # general_geometry keeps refusing loop attacks
    from aware_amd.embedding import AWAREEmbedder
    with pytest.raises(NotImplementedError, match="loop_attacks"):
        AWAREEmbedder(loss="push_extremes", verbose=False, loop_attacks=[SHIFT], general_geometry=True)


def test_abi_symbols_and_bad_arguments():
    from aware_amd import _lib, attacks as A
    lib = _lib.load_library()
    assert "aware_frequency_shift" in _lib.SIGNATURES and hasattr(lib, "aware_frequency_shift")
    assert "loop_shift_kernels.hip" in _lib.SOURCES and len(_lib.SIGNATURES["aware_frequency_shift"][1]) == 10
    assert lib.aware_version() == 350
    with open(os.path.join(ROOT, "include", "aware_hip.h")) as f:
        hdr = f.read()
    assert "#define AWARE_LOOP_FREQUENCY_SHIFT 12" in hdr
    assert "int aware_frequency_shift(const float* in, const int* off, const int* len, int B, int max_len, const int* d, const int* p0,\n" in hdr
    seeds = (C.c_uint32 * 1)(0)
    ent = (_lib.LoopAttackEx * 1)(_lib.LoopAttackEx(12, 0.75, (C.c_float * 4)(-7864.0, 7864.0, 0.0, 0.0)))
    assert lib.aware_embed_set_loop_attacks_ex(None, ent, 1, seeds, None, 0, None) == -1          # no handle
    old = (_lib.LoopAttack * 1)(_lib.LoopAttack(12, 7864.0, 1.0))
    assert lib.aware_embed_set_loop_attacks(None, old, 1, seeds, None, 0, None) == -1
    # the stand-alone entry refuses null pointers and sizes out of range before anything touches a device
    p, q = C.c_void_p(256), C.c_void_p(512)                  # never dereferenced: every call below is refused

    def call(ptrs=(p, p, p, p, p, q), B=1, max_len=16000, adjoint=0):
        return lib.aware_frequency_shift(ptrs[0], ptrs[1], ptrs[2], B, max_len, ptrs[3], ptrs[4], adjoint, ptrs[5], None)

    for i in range(6):                                       # each pointer in turn
        ptrs = [p, p, p, p, p, q]
        ptrs[i] = None
        assert call(ptrs) == -1, i
    assert call((p, p, p, p, p, p)) == -1                    # in == out
    for kw in (dict(B=0), dict(B=65536), dict(max_len=0), dict(max_len=(1 << 30) + 1), dict(adjoint=2), dict(adjoint=-1)):
        assert call(**kw) == -1, kw
    assert "FrequencyShift" in A.ATTACKS and A.make_attack("FrequencyShift", hz=50.0).name == "frequency_shift_50.0"
    assert A.FrequencyShift(-20.0, phase=0.25).phase == 0.25
    assert [type(a).__name__ for a in A.config3_attack_stack()] == ["Resample", "LowPassFilter", "GaussianNoise", "PCMBitDepthConversion"]
    assert len(A.reference_attack_list()) == 13
    for kw in (dict(hz=float("nan")), dict(hz=float("inf")), dict(hz=50.0, phase=float("nan"))):
        with pytest.raises(ValueError):
            A.FrequencyShift(**kw)


# ---- 5. the value claim, on the CPU -------------------------------------------------------------------------------------------------
def hilbert_shifts(y, hz_list=CLAIM_HZ, sr=16000):
    """The attacks of the claim on y [4, n] float32: Re(scipy.signal.hilbert(y) e^{j 2 pi hz i / sr}), the FFT analytic signal.
    None of them is the loop's 255-tap operator."""
    from scipy.signal import hilbert
    ya = hilbert(y.astype(np.float64), axis=-1)
    i = np.arange(y.shape[-1])
    return {hz: np.real(ya * np.exp(2j * np.pi * hz / sr * i)).astype(np.float32) for hz in hz_list}


def test_shift_in_the_loop_survives_frequency_shifts(value_setup):
    """Four 1 s clips, 400 steps, seeds 0..3: BER under constant frequency shifts of -100, -50, -20, -10, +10, +20, +50 and +100 Hz
    made with scipy.signal.hilbert, of the plain embedding and of the embedding with frequency_shift(hz 120, prob 0.75) inside the
    loop.  Clean 0 % for both, the plain mean at least 20 %, the aware mean at most a quarter of it.  Measured with this
    restatement: plain 47.5 / 50 / 23.75 / 0 / 0 / 35 / 48.75 / 55 %, mean 32.5 %; aware 0 % under all eight; clean 0 % for both;
    SNR 15.8 against 15.5 dB."""
    plain, audio, bits, wm, y0 = value_setup
    y1 = AttackedEmbedder(AWARE_CHAIN, [0, 1, 2, 3]).embed(audio, wm)[0].numpy()
    clean0, clean1 = ber(plain, bits, y0), ber(plain, bits, y1)
    b0 = {hz: ber(plain, bits, v) for hz, v in hilbert_shifts(y0).items()}
    b1 = {hz: ber(plain, bits, v) for hz, v in hilbert_shifts(y1).items()}
    for hz in b0:
        print(f"shift {hz:+6.0f} Hz   plain {b0[hz]:6.2f} %   shift-aware {b1[hz]:6.2f} %")
    m0, m1 = float(np.mean(list(b0.values()))), float(np.mean(list(b1.values())))
    print(f"clean BER plain {clean0:.2f} % / shift-aware {clean1:.2f} %; mean over the eight: plain {m0:.2f} % / aware {m1:.2f} %; "
          f"SNR against the host: plain {snr_db(audio, y0):.1f} dB / aware {snr_db(audio, y1):.1f} dB")
    assert clean0 == 0.0 and clean1 == 0.0
    assert m0 >= 20.0
    assert m1 <= 0.25 * m0
