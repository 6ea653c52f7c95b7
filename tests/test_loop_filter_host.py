"""Band filters inside the embed loop (EXTENSION, chain kind 9): the torch restatement of aware_amd/embedding/loop_attacks.py
against a plain loop over the definition, its adjoint, its draw and its place in a chain, the parser in Python and in C
(csrc/loop_chain.hpp through tests/host_sim/loop_chain_check on the CPU), the card keys, the ABI, and the value claim on the CPU:
what a band filter in the loop buys under Butterworth channels that cut into the embedding band, through the oracle's embed loop.
No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, make_clip  # noqa: F401
from aware_amd.embedding import loop_attacks as LA
from test_loop_attacks_host import AttackedEmbedder, _chain_case, _dims_case, _golden, ber, value_setup  # noqa: F401
from test_loop_gain_host import snr_db

ALL4 = ["lowpass", "highpass", "bandpass", "bandstop"]
AWARE_CHAIN = [{"kind": "band_filter", "response": ALL4, "freq": [600.0, 3800.0], "min_width": 400.0, "prob": 0.75}]
FIL = {"kind": "band_filter", "response": "lowpass", "freq": 1000.0}
NOISE = {"kind": "gaussian_noise", "snr_db": 10.0}
W = 1638                                                     # round(65536 * 400 / 16000)
EDGES = [1, 2458, 16384, 32767 - W]


# ---- 1. the model -------------------------------------------------------------------------------------------------------------------
def plain_lowpass(c):
    """lp_c[k], k = -127..127, tap by tap from the issue's definition."""
    out = []
    for k in range(-127, 128):
        if k == 0:
            out.append(c / 32768.0)
            continue
        w = 0.54 + 0.46 * math.cos(math.pi * k / 127)
        out.append(w * math.sin(2.0 * math.pi * ((c * abs(k)) % 65536) / 65536.0) / (math.pi * abs(k)))
    return out


def plain_taps(response, c1, c2):
    delta = [1.0 if k == 0 else 0.0 for k in range(-127, 128)]
    l1 = plain_lowpass(c1)
    if response == 1:
        return l1
    if response == 2:
        return [d - a for d, a in zip(delta, l1)]
    band = [b - a for a, b in zip(l1, plain_lowpass(c2))]
    return band if response == 4 else [d - v for d, v in zip(delta, band)]


def plain_filter(x, h):
    """z[i] = sum_k h[k] x[i - k], x zero outside the clip, sample by sample."""
    n = len(x)
    return [math.fsum(h[k + 127] * x[i - k] for k in range(-127, 128) if 0 <= i - k < n) for i in range(n)]


@pytest.mark.parametrize("response", [1, 2, 4, 8])
@pytest.mark.parametrize("c", EDGES)
def test_taps_are_the_definition(response, c):
    c2 = c + W
    want = np.array(plain_taps(response, c, c2))
    h64 = LA.filter_taps(response, c, c2)
    assert h64.dtype == np.float64 and h64.shape == (255,)
    np.testing.assert_allclose(h64, want, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(h64, h64[::-1])                                  # symmetric: the operator is its own adjoint
    h32 = LA.filter_taps(response, c, c2, np.float32)
    assert h32.dtype == np.float32
    assert np.abs(h32.astype(np.float64) - want).max() <= 1e-6
    # a low-pass row passes DC: its taps sum to about 1 wherever the edge clears the window's main lobe
    if c >= 2458:
        assert abs(sum(plain_lowpass(c)) - 1.0) < 2e-3
    # complementary pairs add up to delta exactly
    delta = np.zeros(255)
    delta[127] = 1.0
    np.testing.assert_array_equal(LA.filter_taps(1, c, c) + LA.filter_taps(2, c, c), delta)
    np.testing.assert_allclose(LA.filter_taps(4, c, c2) + LA.filter_taps(8, c, c2), delta, rtol=0, atol=1e-16)
    with pytest.raises(ValueError):
        LA.filter_taps(3, c, c2)
    with pytest.raises(ValueError):
        LA.filter_taps(1, 32768, c2)


@pytest.mark.parametrize("n", [100, 254, 255, 4099])
def test_band_filter_is_the_definition(n):
    """Two lengths shorter than the taps, one of exactly their count, one of several tiles of any kernel."""
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n)
    for response, c in ((1, 2458), (2, 16384), (4, 1), (8, 32767 - W)):
        c2 = c + W
        z = LA.band_filter(torch.from_numpy(x), response, c, c2).numpy()
        step = 1 if n < 1000 else 97                                              # the long clip at a stride, and at both ends
        idx = sorted(i for i in set(range(0, n, step)) | set(range(130)) | set(range(n - 130, n)) if 0 <= i < n)
        h = plain_taps(response, c, c2)
        want = plain_filter(list(x), h) if n < 1000 else None
        for i in idx:
            w = want[i] if want is not None else math.fsum(h[k + 127] * x[i - k] for k in range(-127, 128) if 0 <= i - k < n)
            assert abs(z[i] - w) <= 1e-12, (n, response, i)
    z32 = LA.band_filter(torch.from_numpy(x).float(), 4, 2458, 9000)
    assert z32.dtype == torch.float32 and z32.shape == (n,)
    rag = LA.band_filter([torch.from_numpy(x), torch.from_numpy(x[:50])], [1, 8], [2458, 3000], [2458, 9000])
    assert [r.shape[0] for r in rag] == [n, 50]
    np.testing.assert_array_equal(rag[0].numpy(), LA.band_filter(torch.from_numpy(x), 1, 2458, 2458).numpy())


@pytest.mark.parametrize("response", [1, 2, 4, 8])
def test_the_operator_is_its_own_adjoint(response):
    rng = np.random.default_rng(7 + response)
    for n in (100, 300, 4099):
        x, w = torch.from_numpy(rng.standard_normal(n)), torch.from_numpy(rng.standard_normal(n))
        lhs = float(torch.dot(LA.band_filter(x, response, 2458, 9000), w))
        rhs = float(torch.dot(x, LA.band_filter(w, response, 2458, 9000)))
        assert abs(lhs - rhs) <= 1e-12 * (1.0 + abs(lhs)), (n, lhs, rhs)
    x = torch.from_numpy(rng.standard_normal(300)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: LA.band_filter(v, response, 2458, 9000), (x,), eps=1e-6, atol=1e-7)


# ---- 2. the draw and the chain ------------------------------------------------------------------------------------------------------
def test_draws_stay_in_range_and_differ():
    chain = LA.parse_chain(AWARE_CHAIN)
    c_lo, c_hi, w_min = LA.filter_range(chain[0], 16000)
    assert (c_lo, c_hi, w_min) == (2458, 15565, W) and LA.filter_mask(chain[0]) == 15
    assert LA.device_entries_ex(chain, 16000) == [(9, 0.75, [15.0, 2458.0, 15565.0, 1638.0])]
    seen, draws = set(), []
    for step in range(300):
        r = LA.entry_draw(3, step, 0)
        rs, c1, c2 = LA.filter_draw(chain[0], r, 16000)
        seen.add(rs)
        draws.append((rs, c1, c2))
        assert rs in (1, 2, 4, 8) and c_lo <= c1 <= c_hi
        if rs >= 4:
            assert c1 + w_min <= c2 <= c_hi + w_min and c2 <= LA.MAX_EDGE
        else:
            assert c2 == c1
        # the definition, in Python integers
        e1 = c_lo + ((int(r[1]) * (c_hi - c_lo + 1)) >> 32)
        e2 = c_lo + ((int(r[2]) * (c_hi - c_lo + 1)) >> 32)
        bit = [1, 2, 4, 8][(int(r[3]) * 4) >> 32]
        lo, hi = min(e1, e2), max(e1, e2)
        assert (rs, c1, c2) == ((bit, e1, e1) if bit < 4 else (bit, lo, max(hi, lo + w_min)))
    assert seen == {1, 2, 4, 8} and len(set(draws)) > 290
    # the response is the chosen set bit of the mask, counted from the lowest
    two = LA.parse_chain([dict(AWARE_CHAIN[0], response=["bandstop", "highpass"])])[0]
    assert two["response"] == ["highpass", "bandstop"] and LA.filter_mask(two) == 10
    for step in range(50):
        r = LA.entry_draw(3, step, 0)
        assert LA.filter_draw(two, r, 16000)[0] == (2 if int(r[3]) < (1 << 31) else 8)
    # min_width is enforced on a narrow range: both edges fall inside 100 Hz, the band is 400 Hz wide
    nar = LA.parse_chain([{"kind": "band_filter", "response": "bandpass", "freq": [1000.0, 1100.0]}])[0]
    for step in range(50):
        rs, c1, c2 = LA.filter_draw(nar, LA.entry_draw(1, step, 0), 16000)
        assert rs == 4 and c2 == c1 + W
    # a scalar freq is a fixed edge
    fix = LA.parse_chain([FIL])[0]
    assert fix["freq"] == [1000.0, 1000.0] and {LA.filter_draw(fix, LA.entry_draw(1, s, 0), 16000) for s in range(20)} == {(1, 4096, 4096)}
    # across step, clip and entry index
    base = LA.filter_draw(chain[0], LA.entry_draw(3, 5, 0), 16000)
    assert base != LA.filter_draw(chain[0], LA.entry_draw(3, 6, 0), 16000)
    assert base != LA.filter_draw(chain[0], LA.entry_draw(4, 5, 0), 16000)
    assert base != LA.filter_draw(chain[0], LA.entry_draw(3, 5, 1), 16000)


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
    # the chain's output is the drawn filter on the clip
    for s in range(5):
        r = LA.entry_draw(9, s, 0)
        z = LA.apply_chain(x, AWARE_CHAIN, [9], s)[0]
        want = LA.band_filter(x[0], *LA.filter_draw(LA.parse_chain(AWARE_CHAIN)[0], r, 16000)) if LA.fires(r[0], 0.75) else x[0]
        assert torch.equal(z, want)
    # noise in front of the filter is coloured with the signal; noise behind it is white and takes its sigma from the filtered signal
    ch = LA.parse_chain([NOISE, FIL])
    z = LA.apply_chain(x, ch, [9], 2)[0]
    noisy = LA.apply_chain(x, [NOISE], [9], 2)[0]
    assert torch.equal(z, LA.band_filter(noisy, 1, 4096, 4096))
    z = LA.apply_chain(x, [FIL, NOISE], [9], 2)[0]
    f = LA.band_filter(x[0], 1, 4096, 4096)
    sigma = math.sqrt(float(np.mean(f.numpy() ** 2)) / 10.0)
    np.testing.assert_allclose((z - f).numpy(), sigma * LA.normal_draws(2000, 9, 2, 1), rtol=0, atol=1e-12)
    # in a mixture: each clip goes through the chain it draws
    mix = [{"weight": 0.5, "chain": AWARE_CHAIN}, {"weight": 0.5, "chain": [NOISE]}]
    xs = torch.from_numpy(np.random.default_rng(1).standard_normal((6, 600)))
    seeds = list(range(6))
    out = LA.apply_mixture(xs, mix, seeds, 3)
    choice = LA.mixture_choices(seeds, 3, [0.5, 0.5])
    for b in range(6):
        assert torch.equal(out[b], LA.apply_chain(xs[b:b + 1], mix[choice[b]]["chain"], [seeds[b]], 3)[0])


# ---- 3. the parsers -----------------------------------------------------------------------------------------------------------------
BAD = [
    ({"kind": "band_filter", "response": "lowpass"}, "freq is required"),
    ({"kind": "band_filter", "freq": 1000.0}, "response is required"),
    ({"kind": "band_filter", "response": "notch", "freq": 1000.0}, "available"),
    ({"kind": "band_filter", "response": ["lowpass", "allpass"], "freq": 1000.0}, "available"),
    ({"kind": "band_filter", "response": [], "freq": 1000.0}, "available"),
    ({"kind": "band_filter", "response": 1, "freq": 1000.0}, "available"),
    ({"kind": "band_filter", "response": "lowpass", "freq": float("nan")}, "finite"),
    ({"kind": "band_filter", "response": "lowpass", "freq": [600.0, float("inf")]}, "finite"),
    ({"kind": "band_filter", "response": "lowpass", "freq": 1000.0, "min_width": float("nan")}, "finite"),
    ({"kind": "band_filter", "response": "lowpass", "freq": [3800.0, 600.0]}, "lo <= hi"),
    ({"kind": "band_filter", "response": "lowpass", "freq": [600.0, 1000.0, 2000.0]}, "neither a number"),
    ({"kind": "band_filter", "response": "lowpass", "freq": "low"}, "neither a number"),
    ({"kind": "band_filter", "response": "lowpass", "freq": 0.0}, "outside"),
    ({"kind": "band_filter", "response": "lowpass", "freq": -100.0}, "outside"),
    ({"kind": "band_filter", "response": "lowpass", "freq": 0.1}, "outside"),                    # rounds to c = 0
    ({"kind": "band_filter", "response": "lowpass", "freq": 7600.0}, "outside"),                 # Nyquist - min_width itself
    ({"kind": "band_filter", "response": "lowpass", "freq": [600.0, 7900.0]}, "outside"),
    ({"kind": "band_filter", "response": "lowpass", "freq": 7000.0, "min_width": 1500.0}, "outside"),
    ({"kind": "band_filter", "response": "lowpass", "freq": 1000.0, "min_width": 0.0}, "min_width"),
    ({"kind": "band_filter", "response": "lowpass", "freq": 1000.0, "min_width": -400.0}, "min_width"),
    ({"kind": "band_filter", "response": "lowpass", "freq": 1000.0, "order": 6}, "unknown key"),
    ({"kind": "band_filter", "response": "lowpass", "freq": 1000.0, "prob": 1.5}, "prob"),
]


@pytest.mark.parametrize("entry,msg", BAD)
def test_parse_chain_refuses(entry, msg):
    with pytest.raises(ValueError, match=msg) as err:
        LA.parse_chain([NOISE, entry])
    assert "loop_attacks[1]" in str(err.value)


def test_parse_chain_accepts_and_keeps_the_tables():
    assert LA.KINDS["band_filter"] == 9 and LA.SPLITTING[6] == "band_filter" and LA.kind_id("band_filter") == 9
    assert list(LA.KINDS)[:8] == list(_golden("loop_chain_messages.json")["entries"]) and LA.KINDS["gain_envelope"] == 8 and "gain_envelope" not in LA.SPLITTING
    assert LA.SPLITTING[:6] == ("reverberation", "speed_change", "time_stretch", "pitch_shift", "phase_vocoder", "delete_samples")
    p = LA.parse_chain([{"kind": "band_filter", "response": "bandstop", "freq": [500.0, 1500.0]}])
    assert p == [{"kind": "band_filter", "prob": 1.0, "response": ["bandstop"], "freq": [500.0, 1500.0], "min_width": 400.0}]
    assert LA.parse_chain(p) == p
    LA.parse_chain([{"kind": "band_filter", "response": "lowpass", "freq": 7599.0}])             # just inside
    LA.parse_chain([{"kind": "band_filter", "response": "lowpass", "freq": 20000.0}], sample_rate=48000)
    with pytest.raises(ValueError, match="outside"):
        LA.parse_chain([{"kind": "band_filter", "response": "lowpass", "freq": 4000.0}], sample_rate=8000)
    LA.check_lengths(LA.parse_chain([FIL]), 16000, [1, 100])                                    # no rule on the lengths
    # the one-split rule against every splitting kind, in either order, and against itself
    table = _golden("loop_chain_messages.json")
    env = {"kind": "gain_envelope", "period": 0.05}
    for kind in LA.SPLITTING[:6]:
        s = table["entries"][kind]
        for chain in ([FIL, s], [s, FIL], [FIL, NOISE, s], [s, env, FIL]):
            with pytest.raises(ValueError, match="not both") as err:
                LA.parse_chain(chain)
            assert "band filter" in str(err.value)
    with pytest.raises(ValueError, match="at most one band filter"):
        LA.parse_chain([FIL, NOISE, FIL])
    for chain in ([NOISE, FIL], [FIL, NOISE], [env, FIL, env, NOISE], [table["entries"]["sample_suppression"], FIL]):
        assert [a["kind"] for a in LA.parse_chain(chain)] == [a["kind"] for a in chain]
    with pytest.raises(ValueError, match="at most 4"):
        LA.parse_chain([NOISE, NOISE, FIL, NOISE, NOISE])
    LA.parse_mixture([{"weight": 0.5, "chain": AWARE_CHAIN}, {"weight": 0.5, "chain": [table["entries"]["reverberation"]]}])
    with pytest.raises(ValueError, match=r"loop_attack_mixture\[1\]"):
        LA.parse_mixture([{"weight": 0.5, "chain": [NOISE]}, {"weight": 0.5, "chain": [FIL, FIL]}])


def test_c_parser_on_the_cpu():
    """csrc/loop_chain.hpp through tests/host_sim/loop_chain_check (built without HIP): rc 0 exactly where parse_chain accepts,
    -1 for each bad parameter, for a fifth entry, beside every other splitting kind and through the older entry point; the byte
    count of a chain with the kind is that of the same chain with a sample deletion in its place."""
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

    fixture = _golden("loop_chains_sha256.json")
    table = _golden("loop_chain_messages.json")
    one = {k: LA.device_entries_ex(LA.parse_chain([a]), 16000)[0] for k, a in table["entries"].items()}
    BF = LA.device_entries_ex(LA.parse_chain(AWARE_CHAIN), 16000)[0]
    assert BF == (9, 0.75, [15.0, 2458.0, 15565.0, 1638.0])
    EV, NO, DS = (8, 0.75, [800.0, 8000.0, 0.25]), one["gaussian_noise"], (7, 0.75, [16.0, 512.0, 1.0])
    for ws in fixture["workspace"]:
        dims = _dims_case(ws["dims"])
        # accepted: alone, with noise, suppression and envelopes on either side; each with the bytes of its deletion twin
        chains = [[BF], [NO, BF], [BF, NO], [EV, BF, EV, NO], [one["sample_suppression"], BF, NO], [NO, EV, NO, BF]]
        twins = [[DS if e is BF else e for e in c] for c in chains]
        got = run(dims + "".join(_chain_case(c) for c in chains) + "".join(_chain_case(c) for c in twins))
        for c, (rc, nbytes), (rc2, nbytes2) in zip(chains, got[:len(chains)], got[len(chains):]):
            assert rc == 0 and rc2 == 0 and nbytes == nbytes2 > 0, (c, rc, nbytes, nbytes2)
        # the parameters at their limits
        ok = [(9, 1.0, [1.0, 1.0, 1.0, 1.0]), (9, 0.0, [15.0, 1.0, 32766.0, 1.0]), (9, 1.0, [8.0, 16384.0, 16384.0, 16383.0])]
        assert [rc for rc, _ in run(dims + "".join(_chain_case([e]) for e in ok))] == [0, 0, 0]
        # refused: every bad parameter, a fifth entry, the older entry point
        nan, inf = float("nan"), float("inf")
        bad = [(9, 1.0, [0.0, 2458.0, 15565.0, 1638.0]), (9, 1.0, [16.0, 2458.0, 15565.0, 1638.0]), (9, 1.0, [1.5, 2458.0, 15565.0, 1638.0]),
               (9, 1.0, [15.0, 0.0, 15565.0, 1638.0]), (9, 1.0, [15.0, 2458.5, 15565.0, 1638.0]), (9, 1.0, [15.0, 15565.0, 2458.0, 1638.0]),
               (9, 1.0, [15.0, 2458.0, 15565.5, 1638.0]), (9, 1.0, [15.0, 2458.0, 15565.0, 0.0]), (9, 1.0, [15.0, 2458.0, 15565.0, 1638.5]),
               (9, 1.0, [15.0, 2458.0, 31130.0, 1638.0]), (9, 1.0, [15.0, 2458.0, 32767.0, 1.0]), (9, 1.0, [nan, 2458.0, 15565.0, 1638.0]),
               (9, 1.0, [15.0, nan, 15565.0, 1638.0]), (9, 1.0, [15.0, 2458.0, inf, 1638.0]), (9, 1.0, [15.0, 2458.0, 15565.0, nan]),
               (9, 1.5, BF[2]), (9, nan, BF[2]), (9, 1.0, [800.0, 8000.0, 0.0, 0.0]), (9, 1.0, [0.0]), (10, 1.0, BF[2])]
        assert [rc for rc, _ in run(dims + "".join(_chain_case([e]) for e in bad))] == [-1] * len(bad)
        assert run(dims + _chain_case([NO, NO, BF, NO, NO]))[0] == (-1, 0)
        assert [rc for rc, _ in run(dims + _chain_case([BF], ex=0) + _chain_case([NO, BF], ex=0))] == [-1, -1]
        # beside every other splitting kind, in either order and with an element-wise entry between them, and beside itself:
        # refused, and sized as the chain was sized before the kind existed (the other kind decides)
        for k in LA.SPLITTING[:6]:
            got = run(dims + "".join(_chain_case(c) for c in ([BF, one[k]], [one[k], BF], [one[k], EV, BF], [one[k]])))
            assert [rc for rc, _ in got[:3]] == [-1, -1, -1], k
            assert got[0][1] == got[1][1] == got[3][1] > 0, k
        got = run(dims + _chain_case([BF, NO, BF]) + _chain_case([DS, NO, NO]))
        assert got[0][0] == -1 and got[0][1] == got[1][1]
        # older chains carve what they carved
        for name, chain in (("noise", [NO]), ("delete", None)):
            if name in ws["bytes"] and chain is not None:
                assert run(dims + _chain_case(chain))[0] == (0, ws["bytes"][name])


# ---- 4. the surface -----------------------------------------------------------------------------------------------------------------
def test_card_keys_reach_the_embedder(tmp_path):
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        text = f.read()
    card = yaml.safe_load(text)
    assert "loop_attacks" not in card and "loop_attack_mixture" not in card              # the committed card keeps its behaviour
    line = "# loop_attacks: [{kind: band_filter, response: [lowpass, highpass, bandpass, bandstop], freq: [600.0, 3800.0], min_width: 400.0, prob: 0.75}]"
    assert line in text
    card["loop_attacks"] = yaml.safe_load(line[2:])["loop_attacks"] + [{"kind": "gaussian_noise", "snr_db": 20.0}]
    card["loop_attack_seed"] = 5
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.loop_attacks == [{"kind": "band_filter", "prob": 0.75, "response": ALL4, "freq": [600.0, 3800.0], "min_width": 400.0},
                                {"kind": "gaussian_noise", "prob": 1.0, "snr_db": 20.0}]
    assert emb.loop_attack_seed == 5
    del card["loop_attacks"]
    card["loop_attack_mixture"] = [{"weight": 0.5, "chain": [{"kind": "band_filter", "response": "lowpass", "freq": 800.0}]},
                                   {"weight": 0.5, "chain": [{"kind": "sample_suppression", "seconds": 0.3}]}]
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.loop_attack_mixture[0] == {"weight": 0.5, "chain": [{"kind": "band_filter", "prob": 1.0, "response": ["lowpass"],
                                                                     "freq": [800.0, 800.0], "min_width": 400.0}]}
    del card["loop_attack_mixture"]
    card["loop_attacks"] = [{"kind": "band_filter", "response": "lowpass", "freq": 7900.0}]
    p.write_text(yaml.safe_dump(card))
    assert load(str(p)) is None                               # a stage that fails is reported as None, as everywhere in load()


def test_abi_symbols_and_bad_arguments():
    from aware_amd import _lib, attacks as A
    lib = _lib.load_library()
    assert "aware_band_filter" in _lib.SIGNATURES and hasattr(lib, "aware_band_filter")
    assert "loop_filter_kernels.hip" in _lib.SOURCES and len(_lib.SIGNATURES["aware_band_filter"][1]) == 11
    assert lib.aware_version() == 350
    with open(os.path.join(ROOT, "include", "aware_hip.h")) as f:
        hdr = f.read()
    assert "#define AWARE_LOOP_BAND_FILTER 9" in hdr and "int aware_band_filter(const float* in, const int* off" in hdr
    seeds = (C.c_uint32 * 1)(0)
    ent = (_lib.LoopAttackEx * 1)(_lib.LoopAttackEx(9, 0.75, (C.c_float * 4)(15.0, 2458.0, 15565.0, 1638.0)))
    assert lib.aware_embed_set_loop_attacks_ex(None, ent, 1, seeds, None, 0, None) == -1          # no handle
    old = (_lib.LoopAttack * 1)(_lib.LoopAttack(9, 15.0, 1.0))
    assert lib.aware_embed_set_loop_attacks(None, old, 1, seeds, None, 0, None) == -1
    # the stand-alone entry refuses null pointers and sizes out of range before anything touches a device
    p, q = C.c_void_p(256), C.c_void_p(512)                  # never dereferenced: every call below is refused

    def call(ptrs=(p, p, p, p, p, p, q), B=1, max_len=16000, taps=None):
        return lib.aware_band_filter(ptrs[0], ptrs[1], ptrs[2], B, max_len, ptrs[3], ptrs[4], ptrs[5], ptrs[6], taps, None)

    for i in range(7):                                       # each pointer in turn; the taps may be null
        ptrs = [p, p, p, p, p, p, q]
        ptrs[i] = None
        assert call(ptrs) == -1, i
    assert call((p, p, p, p, p, p, p)) == -1                 # in == out
    for kw in (dict(B=0), dict(B=65536), dict(max_len=0), dict(max_len=(1 << 30) + 1)):
        assert call(**kw) == -1, kw
    assert "BandFilter" in A.ATTACKS and A.make_attack("BandFilter", response="lowpass", freq=800.0).name == "band_filter_lowpass_800.0"
    assert [type(a).__name__ for a in A.config3_attack_stack()] == ["Resample", "LowPassFilter", "GaussianNoise", "PCMBitDepthConversion"]
    assert len(A.reference_attack_list()) == 13
    for kw in (dict(response="notch", freq=800.0), dict(response="lowpass", freq=800.0, freq_hi=900.0), dict(response="bandpass", freq=800.0),
               dict(response="bandpass", freq=900.0, freq_hi=800.0), dict(response="lowpass", freq=float("nan")), dict(response="highpass", freq=0.0)):
        with pytest.raises(ValueError):
            A.BandFilter(**kw)


# ---- 5. the value claim, on the CPU -------------------------------------------------------------------------------------------------
def butterworth_attacks(y):
    """The six attacks of the claim on y [4, n] float32 at 16 kHz: scipy Butterworth designs as attacks.py makes them, causal
    (lfilter, with phase distortion) but for the band-stop, which is filtfilt.  None of them is the loop's zero-phase FIR."""
    from scipy.signal import butter, filtfilt, lfilter
    y64 = y.astype(np.float64)

    def lf(order, wn, btype):
        b, a = butter(order, wn, btype=btype, fs=16000)
        return lfilter(b, a, y64, axis=-1).astype(np.float32)

    b, a = butter(4, [500.0, 1500.0], btype="bandstop", fs=16000)
    return {"low-pass 800 Hz, order 6": lf(6, 800.0, "low"), "low-pass 1000 Hz, order 6": lf(6, 1000.0, "low"),
            "high-pass 3500 Hz, order 4": lf(4, 3500.0, "high"), "band-pass 1000-1500 Hz, order 4": lf(4, [1000.0, 1500.0], "bandpass"),
            "band-pass 2500-3500 Hz, order 4": lf(4, [2500.0, 3500.0], "bandpass"),
            "band-stop 500-1500 Hz, order 4, filtfilt": filtfilt(b, a, y64, axis=-1).astype(np.float32)}


def test_filter_in_the_loop_survives_band_limited_channels(value_setup):
    """Four 1 s clips, 400 steps, seeds 0..3: BER under six Butterworth channels that cut into the 500-4000 Hz embedding band
    (low-pass 800 and 1000 Hz order 6, high-pass 3500 Hz order 4, band-pass 1000-1500 and 2500-3500 Hz order 4, all causal;
    band-stop 500-1500 Hz order 4, zero-phase) of the plain embedding and of the embedding with band_filter(all four responses,
    freq 600-3800 Hz, min_width 400 Hz, prob 0.75) inside the loop.  Clean 0 % for both, the plain mean at least 10 %, the aware
    mean at most half of it.  Measured with this restatement: plain 21.25 / 7.5 / 12.5 / 20 / 26.25 / 17.5 %, mean 17.5 %; aware
    0 % under all six; clean 0 % for both; SNR 15.8 against 14.8 dB."""
    plain, audio, bits, wm, y0 = value_setup
    y1 = AttackedEmbedder(AWARE_CHAIN, [0, 1, 2, 3]).embed(audio, wm)[0].numpy()
    clean0, clean1 = ber(plain, bits, y0), ber(plain, bits, y1)
    a0, a1 = butterworth_attacks(y0), butterworth_attacks(y1)
    b0 = {k: ber(plain, bits, v) for k, v in a0.items()}
    b1 = {k: ber(plain, bits, v) for k, v in a1.items()}
    for k in b0:
        print(f"{k:42s} plain {b0[k]:6.2f} %   filter-aware {b1[k]:6.2f} %")
    m0, m1 = float(np.mean(list(b0.values()))), float(np.mean(list(b1.values())))
    print(f"clean BER plain {clean0:.2f} % / filter-aware {clean1:.2f} %; mean over the six: plain {m0:.2f} % / aware {m1:.2f} %; "
          f"SNR against the host: plain {snr_db(audio, y0):.1f} dB / aware {snr_db(audio, y1):.1f} dB")
    assert clean0 == 0.0 and clean1 == 0.0
    assert m0 >= 10.0
    assert m1 <= 0.5 * m0
