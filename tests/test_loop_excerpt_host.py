"""The tiled excerpt inside the embed loop (EXTENSION, chain kind 10): the torch restatement of aware_amd/embedding/loop_attacks.py
(excerpt_range, excerpt_draw, excerpt_tile, excerpt_tile_adjoint, apply_chain) against a plain loop over the definition, its
adjoint against the inner product, autograd and an explicit float32 sum over ascending periods, its draw and its place in a
chain and a mixture, the parser in Python and in C (csrc/loop_chain.hpp through tests/host_sim/loop_chain_check on the CPU), the
card keys, the ABI, and the value claim on the CPU: what the kind buys when a detector is handed an excerpt of half a second or
less, through the oracle's embed loop.  No GPU."""
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

AWARE_CHAIN = [{"kind": "excerpt", "seconds": [0.1875, 0.625], "prob": 0.75}]
EX = {"kind": "excerpt", "seconds": [0.1875, 0.625]}
NOISE = {"kind": "gaussian_noise", "snr_db": 10.0}
SUP = {"kind": "sample_suppression", "seconds": 0.3}
FIL = {"kind": "band_filter", "response": "lowpass", "freq": 1000.0}
STARTS = [0, 512, 1024, 2048, 3000, 5000, 7777]


# ---- 1. the model -------------------------------------------------------------------------------------------------------------------
def plain_tile(x, start, L):
    """z[i] = x[start + (i mod L)], sample by sample."""
    return [x[start + (i % L)] for i in range(len(x))]


def plain_adjoint(gz, start, L, add=lambda a, b: a + b):
    """gx[i] = sum_m gz[(i - start) + m L] over ascending m while the index is below n, for start <= i < start + L; 0 outside.
    The accumulator starts as the first term."""
    n = len(gz)
    out = []
    for i in range(n):
        if not start <= i < start + L:
            out.append(type(gz[0])(0.0))
            continue
        q = i - start
        acc = gz[q]
        q += L
        while q < n:
            acc = add(acc, gz[q])
            q += L
        out.append(acc)
    return out


def cases(n):
    """(start, L as asked, L as clamped) over L in {1024, n - 1, n, n + 5} and start in {0, n - L}."""
    out = []
    for want in (1024, n - 1, n, n + 5):
        L = min(want, n)
        for start in sorted({0, n - L}):
            out.append((start, want, L))
    return out


@pytest.mark.parametrize("n", [1024, 1025, 4099])
def test_excerpt_tile_is_the_definition(n):
    x = unit_clip(3, n)
    for start, want, L in cases(n):
        z = LA.excerpt_tile(x, start, L)
        assert z.dtype == torch.float64 and z.shape == (n,)
        np.testing.assert_array_equal(z.numpy(), np.array(plain_tile(x.numpy(), start, L)))
        z32 = LA.excerpt_tile(x.float(), start, L)
        assert z32.dtype == torch.float32
        np.testing.assert_array_equal(z32.numpy(), np.array(plain_tile(x.float().numpy(), start, L), dtype=np.float32))
        if L == n:
            assert z is x and LA.excerpt_tile_adjoint(x, start, L) is x                     # the identity, in both directions
    xb = torch.stack([x, -2 * x])                                                           # the operator acts on the last axis
    np.testing.assert_array_equal(LA.excerpt_tile(xb, 17, 300)[1].numpy(), -2 * np.array(plain_tile(x.numpy(), 17, 300)))
    for start, L in ((-1, 5), (0, n + 1), (n - 3, 4), (0, 0)):
        with pytest.raises(ValueError):
            LA.excerpt_tile(x, start, L)
        with pytest.raises(ValueError):
            LA.excerpt_tile_adjoint(x, start, L)
    # a ragged list, with a start and a length each
    clips = [unit_clip(1, 1025), unit_clip(2, 4099)]
    out = LA.excerpt_tile(clips, [1, 99], [1024, 2000])
    assert isinstance(out, list) and [len(o) for o in out] == [1025, 4099]
    np.testing.assert_array_equal(out[1].numpy(), np.array(plain_tile(clips[1].numpy(), 99, 2000)))
    back = LA.excerpt_tile_adjoint(clips, [1, 99], [1024, 2000])
    np.testing.assert_array_equal(back[1].numpy(), np.array(plain_adjoint(clips[1].numpy(), 99, 2000)))


@pytest.mark.parametrize("n", [1024, 1025, 4099])
def test_adjoint_is_the_transpose(n):
    """<z, w> = <x, adjoint(w)> in float64, and the adjoint is what autograd gives."""
    x = unit_clip(7, n)
    w = torch.from_numpy(np.cos(0.37 * np.arange(n)) * np.linspace(0.2, 1.0, n))
    for start, want, L in cases(n) + [(3, 0, 400), (n - 333, 0, 333), (11, 0, 1)]:
        z, gx = LA.excerpt_tile(x, start, L), LA.excerpt_tile_adjoint(w, start, L)
        lhs, rhs = float((z * w).sum()), float((x * gx).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (start, L, lhs, rhs)
        np.testing.assert_array_equal(gx.numpy(), np.array(plain_adjoint(w.numpy(), start, L)))
        xg = x.clone().requires_grad_(True)
        (LA.excerpt_tile(xg, start, L) * w).sum().backward()
        np.testing.assert_allclose(xg.grad.numpy(), gx.numpy(), rtol=0, atol=1e-13)         # autograd's order of the sum is its own


def test_gradcheck():
    x = unit_clip(5, 37).requires_grad_(True)
    for start, L in ((0, 37), (0, 10), (5, 10), (27, 10), (4, 33), (36, 1)):
        assert torch.autograd.gradcheck(lambda v: LA.excerpt_tile(v, start, L), (x,), eps=1e-6, atol=1e-8)


@pytest.mark.parametrize("n", [1024, 1025, 4099])
def test_float32_adjoint_is_the_ascending_sum_bit_for_bit(n):
    gz = (unit_clip(9, n).float() * 3.7).numpy()
    add = lambda a, b: np.float32(a + b)                                                    # one rounded float32 addition
    for start, want, L in cases(n) + [(3, 0, 400), (n - 333, 0, 333), (5, 0, 1000)]:
        got = LA.excerpt_tile_adjoint(torch.from_numpy(gz), start, L).numpy()
        assert got.dtype == np.float32
        ref = np.array(plain_adjoint(list(gz), start, L, add), dtype=np.float32)
        np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))
        assert not np.any(np.signbit(got[:start])) and not np.any(np.signbit(got[start + L:]) & (got[start + L:] == 0))


# ---- 2. the draw --------------------------------------------------------------------------------------------------------------------
def test_draw_is_the_definition_and_in_range():
    e = LA.parse_chain([EX])[0]
    assert LA.excerpt_range(e, 16000) == (3000, 10000)
    seen = set()
    for seed in range(4):
        for step in range(40):
            for j in range(3):
                r = LA.entry_draw(seed, step, j)
                for ny in (15872, 7936, 3072, 2999, 513):
                    start, L = LA.excerpt_draw(e, r, ny, 16000)
                    want = min(3000 + ((int(r[2]) * 7001) >> 32), ny)
                    assert L == want and start == (int(r[1]) * (ny - want + 1)) >> 32
                    assert 1 <= L <= ny and 0 <= start <= ny - L
                    assert LA.excerpt_draw(e, r, ny, 16000, on=False) == (0, ny)
                seen.add((seed, step, j, LA.excerpt_draw(e, r, 15872, 16000)))
    by = lambda key: len({d for (sd, s, j, d) in seen if key(sd, s, j)})
    assert by(lambda sd, s, j: sd == 0 and j == 0) >= 39                                    # across steps
    assert by(lambda sd, s, j: s == 0 and j == 0) == 4 and by(lambda sd, s, j: sd == 0 and s == 0) == 3      # clips, entries
    # both ends of both ranges
    lo, hi = np.array([0, 0, 0, 0], dtype=np.uint32), np.array([0, 0xFFFFFFFF, 0xFFFFFFFF, 0], dtype=np.uint32)
    assert LA.excerpt_draw(e, lo, 15872, 16000) == (0, 3000) and LA.excerpt_draw(e, hi, 15872, 16000) == (15872 - 10000, 10000)
    assert LA.excerpt_draw(e, hi, 4096, 16000) == (0, 4096)                                 # a clip shorter than the draw: left alone
    fixed = LA.parse_chain([{"kind": "excerpt", "seconds": 0.5}])[0]
    assert LA.excerpt_range(fixed, 16000) == (8000, 8000) and LA.excerpt_draw(fixed, hi, 15872, 16000) == (7872, 8000)


def test_probability_and_identity():
    x = unit_clip(4, 15872)[None]
    for step in range(5):
        assert torch.equal(LA.apply_chain(x, [dict(EX, prob=0.0)], [9], step), x)
        r = LA.entry_draw(9, step, 0)
        start, L = LA.excerpt_draw(LA.parse_chain([EX])[0], r, 15872, 16000)
        np.testing.assert_array_equal(LA.apply_chain(x, [dict(EX, prob=1.0)], [9], step)[0].numpy(),
                                      np.array(plain_tile(x[0].numpy(), start, L)))
    # every L of the range is shorter than this clip, so a step that fires changes it
    fired = sum(int(not torch.equal(LA.apply_chain(x, [dict(EX, prob=0.75)], [2], s), x)) for s in range(400))
    assert fired == sum(int(LA.fires(LA.entry_draw(2, s, 0)[0], 0.75)) for s in range(400))
    assert abs(fired - 300) <= 3 * math.sqrt(400 * 0.75 * 0.25), fired                      # 0.75 +- 3 sigma of 400 draws
    short = unit_clip(4, 2999)[None]                                                        # shorter than L_lo: never touched
    for step in range(8):
        assert torch.equal(LA.apply_chain(short, [dict(EX, prob=1.0)], [1], step), short)


def test_order_with_noise_on_either_side():
    x = unit_clip(6, 15872)[None]
    e = LA.parse_chain([EX])[0]
    start, L = LA.excerpt_draw(e, LA.entry_draw(1, 0, 0), 15872, 16000)
    res = LA.apply_chain(x, [e], [1], 0)[0]
    np.testing.assert_array_equal(res.numpy(), np.array(plain_tile(x[0].numpy(), start, L)))
    # noise behind it: its sigma comes from the tiled signal, and it is not periodic
    both = LA.apply_chain(x, [e, NOISE], [1], 0)[0]
    sigma = np.sqrt(float((res ** 2).mean()) / 10.0)
    np.testing.assert_allclose((both - res).numpy(), sigma * LA.normal_draws(15872, 1, 0, 1), atol=1e-12)
    # noise in front: it is tiled with the clip (the draw is entry 1's)
    front = LA.apply_chain(x, [NOISE, e], [1], 0)[0]
    noisy = LA.apply_chain(x, [NOISE], [1], 0)[0]
    s1, L1 = LA.excerpt_draw(e, LA.entry_draw(1, 0, 1), 15872, 16000)
    np.testing.assert_array_equal(front.numpy(), np.array(plain_tile(noisy.numpy(), s1, L1)))
    assert (s1, L1) != (start, L)
    # ragged lists keep their container
    clips = [unit_clip(1, 7936), unit_clip(2, 40192)]
    out = LA.apply_chain(clips, [e], [4, 5], 2)
    assert isinstance(out, list) and [len(o) for o in out] == [7936, 40192]
    np.testing.assert_array_equal(out[1].numpy(), LA.apply_chain(clips[1][None], [e], [5], 2)[0].numpy())


def test_inside_a_mixture():
    mix = [{"weight": 0.5, "chain": [EX, NOISE]}, {"weight": 0.3, "chain": [{"kind": "reverberation", "rt60": 0.1}]}]
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
    ({"kind": "excerpt"}, "seconds is required"),
    ({"kind": "excerpt", "prob": 0.5}, "seconds is required"),
    ({"kind": "excerpt", "seconds": 0.5, "at": "start"}, "unknown key"),
    ({"kind": "excerpt", "seconds": 0.5, "snr_db": 10.0}, "unknown key"),
    ({"kind": "excerpt", "seconds": float("nan")}, "finite"),
    ({"kind": "excerpt", "seconds": float("inf")}, "finite"),
    ({"kind": "excerpt", "seconds": [0.2, float("inf")]}, "finite"),
    ({"kind": "excerpt", "seconds": [float("nan"), 0.5]}, "finite"),
    ({"kind": "excerpt", "seconds": [0.5, 0.2]}, "lo <= hi"),
    ({"kind": "excerpt", "seconds": 0.0}, "0 < lo"),
    ({"kind": "excerpt", "seconds": -0.5}, "0 < lo"),
    ({"kind": "excerpt", "seconds": 0.06}, "at least 1024"),                                # 960 samples
    ({"kind": "excerpt", "seconds": [0.0639, 0.5]}, "at least 1024"),                       # 1022 samples
    ({"kind": "excerpt", "seconds": [0.1, 0.2, 0.3]}, "neither a number"),
    ({"kind": "excerpt", "seconds": [0.2]}, "neither a number"),
    ({"kind": "excerpt", "seconds": "short"}, "neither a number"),
    ({"kind": "excerpt", "seconds": 0.5, "prob": 1.5}, "prob"),
]


@pytest.mark.parametrize("entry,msg", BAD)
def test_parse_chain_refuses(entry, msg):
    with pytest.raises(ValueError, match=msg) as err:
        LA.parse_chain([NOISE, entry])
    assert "loop_attacks[1]" in str(err.value)


def test_parse_chain_accepts_and_keeps_the_tables():
    assert LA.KINDS["excerpt"] == 10 and LA.SPLITTING[7] == "excerpt" and LA.kind_id("excerpt") == 10 and LA.MIN_EXCERPT == 1024
    table = _golden("loop_chain_messages.json")
    assert list(LA.KINDS)[:8] == list(table["entries"]) and list(LA.KINDS.values()) == list(range(len(LA.KINDS)))
    assert LA.KINDS["gain_envelope"] == 8 and "gain_envelope" not in LA.SPLITTING and LA.KINDS["band_filter"] == 9 and LA.SPLITTING[6] == "band_filter"
    assert LA.SPLITTING[:6] == ("reverberation", "speed_change", "time_stretch", "pitch_shift", "phase_vocoder", "delete_samples")
    p = LA.parse_chain([{"kind": "excerpt", "seconds": (0.1875, 0.625), "prob": 0.75}])
    assert p == [{"kind": "excerpt", "prob": 0.75, "seconds": [0.1875, 0.625]}] and LA.parse_chain(p) == p
    assert LA.parse_chain([{"kind": "excerpt", "seconds": 0.5}]) == [{"kind": "excerpt", "prob": 1.0, "seconds": [0.5, 0.5]}]
    assert LA.device_entries_ex(p, 16000) == [(10, 0.75, [3000.0, 10000.0, 0.0, 0.0])]
    LA.parse_chain([{"kind": "excerpt", "seconds": 0.064}])                                 # 1024 samples: just inside
    LA.parse_chain([{"kind": "excerpt", "seconds": 0.03}], sample_rate=48000)              # the rule reads the sample rate
    with pytest.raises(ValueError, match="at least 1024"):
        LA.parse_chain([{"kind": "excerpt", "seconds": 0.1}], sample_rate=8000)
    LA.check_lengths(p, 16000, [513, 100])                                                  # no rule on the lengths: a short clip is left alone
    # the one-split rule against every other splitting kind, in either order, and against itself
    env = {"kind": "gain_envelope", "period": 0.05}
    for s in [table["entries"][k] for k in LA.SPLITTING[:6]] + [FIL]:
        for chain in ([EX, s], [s, EX], [EX, NOISE, s], [s, env, EX]):
            with pytest.raises(ValueError, match="not both") as err:
                LA.parse_chain(chain)
            assert "tiled excerpt" in str(err.value)
    with pytest.raises(ValueError, match="at most one tiled excerpt"):
        LA.parse_chain([EX, NOISE, EX])
    for chain in ([NOISE, EX], [EX, NOISE], [env, EX, env, NOISE], [SUP, EX], [NOISE, SUP, EX, NOISE]):
        assert [a["kind"] for a in LA.parse_chain(chain)] == [a["kind"] for a in chain]
    with pytest.raises(ValueError, match="at most 4"):
        LA.parse_chain([NOISE, NOISE, EX, NOISE, NOISE])
    with pytest.raises(ValueError, match="unknown kind") as err:
        LA.parse_chain([{"kind": "excerpts", "seconds": 0.5}])
    assert "excerpt" in str(err.value)
    LA.parse_mixture([{"weight": 0.5, "chain": AWARE_CHAIN}, {"weight": 0.5, "chain": [table["entries"]["reverberation"]]}])
    with pytest.raises(ValueError, match=r"loop_attack_mixture\[1\]"):
        LA.parse_mixture([{"weight": 0.5, "chain": [NOISE]}, {"weight": 0.5, "chain": [EX, EX]}])
    from aware_amd.embedding import AWAREEmbedder
    assert AWAREEmbedder(loss="push_extremes", verbose=False, loop_attacks=[SUP, EX, NOISE]).loop_attacks == LA.parse_chain([SUP, EX, NOISE])
    with pytest.raises(ValueError):
        AWAREEmbedder(loss="push_extremes", verbose=False, loop_attacks=[EX, FIL])


def test_c_parser_on_the_cpu():
    """csrc/loop_chain.hpp through tests/host_sim/loop_chain_check (built without HIP): rc 0 exactly where parse_chain accepts,
    -1 for each bad parameter, for a fifth entry, beside every other splitting kind and through the older entry point; the byte
    count of a chain with the kind is that of the same chain with a sample deletion in its place; older chains keep the bytes
    recorded in tests/golden/loop_chains_sha256.json."""
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
    XC = LA.device_entries_ex(LA.parse_chain(AWARE_CHAIN), 16000)[0]
    assert XC == (10, 0.75, [3000.0, 10000.0, 0.0, 0.0])
    BF = (9, 0.75, [15.0, 2458.0, 15565.0, 1638.0])
    EV, NO, DS = (8, 0.75, [800.0, 8000.0, 0.25]), one["gaussian_noise"], (7, 0.75, [16.0, 512.0, 1.0])
    for ws in fixture["workspace"]:
        dims = _dims_case(ws["dims"])
        # accepted: alone, with noise, suppression and envelopes on either side; each with the bytes of its deletion twin
        chains = [[XC], [NO, XC], [XC, NO], [EV, XC, EV, NO], [one["sample_suppression"], XC, NO], [NO, EV, NO, XC]]
        twins = [[DS if e is XC else e for e in c] for c in chains]
        got = run(dims + "".join(_chain_case(c) for c in chains) + "".join(_chain_case(c) for c in twins))
        for c, (rc, nbytes), (rc2, nbytes2) in zip(chains, got[:len(chains)], got[len(chains):]):
            assert rc == 0 and rc2 == 0 and nbytes == nbytes2 > 0, (c, rc, nbytes, nbytes2)
        # ... and inside a mixture, beside a reverberation chain
        m = run(dims + _mixture_case([([XC, NO], 0.5), ([one["reverberation"]], 0.5)])
                + _mixture_case([([DS, NO], 0.5), ([one["reverberation"]], 0.5)]))
        assert m[0][0] == 0 and m[1][0] == 0 and m[0][1] == m[1][1] > 0
        # the parameters at their limits; a clip shorter than L_lo is no reason to refuse (-2 is the deletion's and the suppression's)
        ok = [(10, 1.0, [1024.0, 1024.0, 0.0, 0.0]), (10, 0.0, [1024.0, 2147483520.0, 0.0, 0.0]), (10, 1.0, [100000.0, 200000.0, 0.0, 0.0])]
        assert [rc for rc, _ in run(dims + "".join(_chain_case([e]) for e in ok))] == [0, 0, 0]
        # refused: every bad parameter, a fifth entry, the older entry point
        nan, inf = float("nan"), float("inf")
        bad = [(10, 1.0, [1023.0, 10000.0, 0.0, 0.0]), (10, 1.0, [0.0, 10000.0, 0.0, 0.0]), (10, 1.0, [-3000.0, 10000.0, 0.0, 0.0]),
               (10, 1.0, [3000.5, 10000.0, 0.0, 0.0]), (10, 1.0, [3000.0, 10000.5, 0.0, 0.0]), (10, 1.0, [10000.0, 3000.0, 0.0, 0.0]),
               (10, 1.0, [3000.0, 2147483648.0, 0.0, 0.0]), (10, 1.0, [3000.0, 10000.0, 1.0, 0.0]), (10, 1.0, [3000.0, 10000.0, 0.0, 1.0]),
               (10, 1.0, [3000.0, 10000.0, -1.0, 0.0]), (10, 1.0, [3000.0, 10000.0, 0.0, 0.5]), (10, 1.0, [nan, 10000.0, 0.0, 0.0]),
               (10, 1.0, [3000.0, nan, 0.0, 0.0]), (10, 1.0, [3000.0, inf, 0.0, 0.0]), (10, 1.0, [3000.0, 10000.0, nan, 0.0]),
               (10, 1.0, [3000.0, 10000.0, 0.0, nan]), (10, 1.5, XC[2]), (10, -0.1, XC[2]), (10, nan, XC[2]), (10, 1.0, BF[2]),
               (10, 1.0, [0.0]), (11, 1.0, XC[2]), (-1, 1.0, XC[2])]
        assert [rc for rc, _ in run(dims + "".join(_chain_case([e]) for e in bad))] == [-1] * len(bad)
        assert run(dims + _chain_case([NO, NO, XC, NO, NO]))[0] == (-1, 0)
        assert [rc for rc, _ in run(dims + _chain_case([XC], ex=0) + _chain_case([NO, XC], ex=0))] == [-1, -1]
        # beside every other splitting kind, in either order and with an element-wise entry between them, and beside itself:
        # refused, and sized as the chain was sized before the kind existed (the other kind decides)
        for other in [one[k] for k in LA.SPLITTING[:6]] + [BF]:
            got = run(dims + "".join(_chain_case(c) for c in ([XC, other], [other, XC], [other, EV, XC], [other])))
            assert [rc for rc, _ in got[:3]] == [-1, -1, -1], other
            assert got[0][1] == got[1][1] == got[3][1] > 0, other
        got = run(dims + _chain_case([XC, NO, XC]) + _chain_case([DS, NO, NO]))
        assert got[0][0] == -1 and got[0][1] == got[1][1]
        # rc 0 exactly where parse_chain accepts: every ordered pair with the kinds of the message table
        for k, a in table["entries"].items():
            for chain, ent in (([EX, a], [XC, one[k]]), ([a, EX], [one[k], XC])):
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
    line = "# loop_attacks: [{kind: excerpt, seconds: [0.1875, 0.625], prob: 0.75}]"
    assert line in text
    card["loop_attacks"] = yaml.safe_load(line[2:])["loop_attacks"] + [{"kind": "gaussian_noise", "snr_db": 20.0}]
    card["loop_attack_seed"] = 5
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.loop_attacks == [{"kind": "excerpt", "prob": 0.75, "seconds": [0.1875, 0.625]},
                                {"kind": "gaussian_noise", "prob": 1.0, "snr_db": 20.0}]
    assert emb.loop_attack_seed == 5
    del card["loop_attacks"]
    card["loop_attack_mixture"] = [{"weight": 0.5, "chain": [{"kind": "excerpt", "seconds": 0.5}]},
                                   {"weight": 0.5, "chain": [{"kind": "sample_suppression", "seconds": 0.3}]}]
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.loop_attack_mixture[0] == {"weight": 0.5, "chain": [{"kind": "excerpt", "prob": 1.0, "seconds": [0.5, 0.5]}]}
    del card["loop_attack_mixture"]
    card["loop_attacks"] = [{"kind": "excerpt", "seconds": 0.05}]
    p.write_text(yaml.safe_dump(card))
    assert load(str(p)) is None                               # a stage that fails is reported as None, as everywhere in load()
    from aware_amd.embedding import AWAREEmbedder
    with pytest.raises(NotImplementedError, match="loop_attacks"):                          # the kind is for the card route
        AWAREEmbedder(frame_length=512, hop_length=128, win_length=512, general_geometry=True, verbose=False, loss="push_extremes",
                      detection_net_cfg={"n_fft": 512}, loop_attacks=AWARE_CHAIN)


def test_abi_symbols_and_bad_arguments():
    from aware_amd import _lib, attacks as A
    lib = _lib.load_library()
    assert "aware_excerpt_tile" in _lib.SIGNATURES and hasattr(lib, "aware_excerpt_tile")
    assert "loop_excerpt_kernels.hip" in _lib.SOURCES and len(_lib.SIGNATURES["aware_excerpt_tile"][1]) == 10
    assert lib.aware_version() == 350
    with open(os.path.join(ROOT, "include", "aware_hip.h")) as f:
        hdr = f.read()
    assert "#define AWARE_LOOP_EXCERPT 10" in hdr and "int aware_excerpt_tile(const float* in, const int* off" in hdr
    with open(os.path.join(ROOT, "aware_amd", "csrc", "loop_limits.hpp")) as f:
        lim = f.read()
    assert "kLoopExcerpt = 10" in lim and "kExcerptMinLen = 1024" in lim
    seeds = (C.c_uint32 * 1)(0)
    ent = (_lib.LoopAttackEx * 1)(_lib.LoopAttackEx(10, 0.75, (C.c_float * 4)(3000.0, 10000.0, 0.0, 0.0)))
    assert lib.aware_embed_set_loop_attacks_ex(None, ent, 1, seeds, None, 0, None) == -1          # no handle
    assert lib.aware_embed_loop_attack_workspace_bytes_ex(None, ent, 1) == 0
    old = (_lib.LoopAttack * 1)(_lib.LoopAttack(10, 3000.0, 1.0))
    assert lib.aware_embed_set_loop_attacks(None, old, 1, seeds, None, 0, None) == -1
    # the stand-alone entry refuses null pointers, sizes out of range and aliasing before anything touches a device
    assert lib.aware_excerpt_tile(None, None, None, 1, 16000, None, None, None, 0, None) == -1
    p, q = C.c_void_p(256), C.c_void_p(512)                  # never dereferenced: every call below is refused
    for i in range(6):                                       # each pointer in turn
        a = [p, p, p, p, p, q]
        a[i] = None
        assert lib.aware_excerpt_tile(a[0], a[1], a[2], 1, 16000, a[3], a[4], a[5], 0, None) == -1, i
    for B, max_len, adjoint in ((0, 16000, 0), (65536, 16000, 0), (-1, 16000, 0), (1, 0, 0), (1, (1 << 30) + 1, 0), (1, 16000, 2),
                                (1, 16000, -1)):
        assert lib.aware_excerpt_tile(p, p, p, B, max_len, p, p, q, adjoint, None) == -1, (B, max_len, adjoint)
    assert lib.aware_excerpt_tile(p, p, p, 1, 16000, p, p, p, 0, None) == -1               # out == in
    assert {"Excerpt", "ExcerptTile", "Cropout"} <= set(A.ATTACKS)
    assert A.make_attack("Excerpt", seconds=0.5).name == "excerpt_0.5_at_0.0"
    assert A.make_attack("ExcerptTile", seconds=0.5, start_seconds=0.25).name == "excerpt_tile_0.5_at_0.25"
    assert [type(a).__name__ for a in A.config3_attack_stack()] == ["Resample", "LowPassFilter", "GaussianNoise", "PCMBitDepthConversion"]
    assert len(A.reference_attack_list()) == 13
    for cls in (A.Excerpt, A.ExcerptTile):
        for kw in (dict(seconds=0.0), dict(seconds=-1.0), dict(seconds=float("nan")), dict(seconds=0.5, start_seconds=-0.1),
                   dict(seconds=0.5, start_seconds=float("inf"))):
            with pytest.raises(ValueError):
                cls(**kw)


# ---- 5. the value claim, on the CPU -------------------------------------------------------------------------------------------------
def slice_table(plain, bits, y, lengths=(12000, 8000, 6000, 4000, 3000)):
    """{L: mean BER % of the plain slices y[:, s:s+L] over the starts of STARTS that fit}."""
    n = y.shape[-1]
    return {L: float(np.mean([ber(plain, bits, y[:, s:s + L]) for s in STARTS if s + L <= n])) for L in lengths}


def slice_mean(plain, bits, y):
    """Mean BER % over every slice of 8000 and of 6000 samples at the starts of STARTS that fits: the figure of the claim."""
    n = y.shape[-1]
    return float(np.mean([ber(plain, bits, y[:, s:s + L]) for L in (8000, 6000) for s in STARTS if s + L <= n]))


def test_excerpt_in_the_loop_survives_excerpting(value_setup):
    """Four 1 s clips, 400 steps, seeds 0..3: BER of plain slices y[:, s:s+L] of 8000 and 6000 samples (0.5 and 0.375 s) at the
    starts 0, 512, 1024, 2048, 3000, 5000 and 7777, every one that fits, of the plain embedding and of the embedding with
    excerpt(seconds 0.1875..0.625, prob 0.75) inside the loop.  Clean 0 % for both, the plain mean at least 10 %, the aware mean
    at most half of it.  The figures measured with this restatement are in DESIGN.md section 32; the kind's limit is a quarter of
    a second (4000 samples), below which it buys little."""
    plain, audio, bits, wm, y0 = value_setup
    y1 = AttackedEmbedder(AWARE_CHAIN, [0, 1, 2, 3]).embed(audio, wm)[0].numpy()
    clean0, clean1 = ber(plain, bits, y0), ber(plain, bits, y1)
    t0, t1 = slice_table(plain, bits, y0), slice_table(plain, bits, y1)
    for L in t0:
        print(f"slices of {L:5d} samples: plain {t0[L]:6.2f} %   excerpt-aware {t1[L]:6.2f} %")
    m0, m1 = slice_mean(plain, bits, y0), slice_mean(plain, bits, y1)
    print(f"clean BER plain {clean0:.2f} % / excerpt-aware {clean1:.2f} %; mean over the slices of 8000 and 6000: plain {m0:.2f} % / "
          f"aware {m1:.2f} %; SNR against the host: plain {snr_db(audio, y0):.1f} dB / aware {snr_db(audio, y1):.1f} dB")
    assert clean0 == 0.0 and clean1 == 0.0
    assert m0 >= 10.0
    assert m1 <= 0.5 * m0
