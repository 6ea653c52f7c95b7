"""Gain envelopes inside the embed loop (EXTENSION, chain kind 8): the torch restatement of aware_amd/embedding/loop_attacks.py
against a plain loop over the definition, its adjoint, its place in a chain, the parser in Python and in C (csrc/loop_chain.hpp
through tests/host_sim/loop_chain_check on the CPU), the card keys, the ABI, and the value claim on the CPU: what an envelope in
the loop buys under fades, tremolo and ducking, through the oracle's embed loop.  No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, make_clip
from oracle import aware_oracle as O
from aware_amd.embedding import loop_attacks as LA
from test_loop_attacks_host import AttackedEmbedder, _chain_case, _dims_case, _golden, ber, unit_clip, value_setup  # noqa: F401

ENV = {"kind": "gain_envelope", "period": 0.05}
AWARE_CHAIN = [{"kind": "gain_envelope", "period": [0.05, 0.5], "prob": 0.75}]
EIGHT = ["gaussian_noise", "sample_suppression", "reverberation", "speed_change", "time_stretch", "pitch_shift", "phase_vocoder",
         "delete_samples"]


# ---- 1. the model -------------------------------------------------------------------------------------------------------------------
def philox_one(c, key, rounds=10):
    """Philox-4x32 on one counter in Python integers: the definition, not the vectorised twin."""
    c0, c1, c2, c3 = c
    k0, k1 = key
    for _ in range(rounds):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def plain_loop(n, seed, step, j, P, ph, floor):
    """g(i) for i < n, sample by sample from the issue's definition."""
    f32 = np.float32
    cache = {}

    def g_k(k):
        if k not in cache:
            w = philox_one((k // 4, step, 16 + j, 0), (seed, 0x5EED))[k % 4]
            u = f32(w >> 8) * f32(2.0 ** -24)
            cache[k] = f32(f32(floor) + f32(f32(1.0) - f32(floor)) * u)
        return cache[k]

    out = np.empty(n, dtype=np.float32)
    for i in range(n):
        pos = i + ph
        k = pos // P
        f = f32(pos - k * P) / f32(P)
        out[i] = f32(g_k(k) + f32(f * f32(g_k(k + 1) - g_k(k))))
    return out


@pytest.mark.parametrize("floor", [0.0, 0.25])
@pytest.mark.parametrize("P", [64, 777, 20000])
@pytest.mark.parametrize("n", [4099, 7937])
def test_model_against_a_plain_loop(n, P, floor):
    """gain_envelope in float32 and float64 against the sample-by-sample definition: the gains bit for bit, the product to a
    rounding; gains within [floor, 1), ph < P, g continuous at the breakpoints (it moves by at most 1 / P per sample)."""
    seed, step, j = 1234567 + n, 3, 2
    r = LA.entry_draw(seed, step, j)
    Pd, ph = LA.envelope_draw({"period": [P / 16000.0 + 1e-9] * 2}, r, 16000)
    assert Pd == P and 0 <= ph < P and ph == (int(r[1]) * P) >> 32
    ref = plain_loop(n, seed, step, j, P, ph, floor)
    g = LA.envelope_curve(n, seed, step, j, P, ph, floor)
    assert g.dtype == np.float32
    np.testing.assert_array_equal(g, ref)
    gk = LA.envelope_gains(seed, step, j, (n - 1 + ph) // P + 2, floor)
    assert gk.dtype == np.float32 and float(gk.min()) >= floor and float(gk.max()) < 1.0
    assert float(g.min()) >= floor and float(g.max()) < 1.0
    assert float(np.abs(np.diff(g.astype(np.float64))).max()) <= (1.0 - floor) / P + 1e-7          # no jump at a breakpoint
    if P < n:
        k0 = -(-ph // P)                                                   # the first breakpoint inside the clip
        np.testing.assert_array_equal(g[k0 * P - ph], gk[k0])             # f = 0 there: the breakpoint's own gain
    x64 = unit_clip(5, n)
    for x in (x64, x64.float()):
        z = LA.gain_envelope(x, seed, step, j, P, ph, floor)
        assert z.dtype == x.dtype and z.shape == x.shape
        np.testing.assert_array_equal(z.numpy(), (x * torch.from_numpy(ref).to(x.dtype)).numpy())
    # the second breakpoint quad comes from the second counter
    assert LA.envelope_gains(seed, step, j, 9, floor)[8] == plain_loop(1, seed, step, j, 64, 8 * 64, floor)[0]


def test_ragged_lists_and_apply_chain():
    clips = [unit_clip(1, 4099), unit_clip(2, 7937).float()]
    out = LA.gain_envelope(clips, [4, 5], 2, 1, 777, 13, 0.25)
    assert isinstance(out, list) and [len(o) for o in out] == [4099, 7937] and [o.dtype for o in out] == [torch.float64, torch.float32]
    np.testing.assert_array_equal(out[1].numpy(), LA.gain_envelope(clips[1], 5, 2, 1, 777, 13, 0.25).numpy())
    # apply_chain draws P and ph itself; a period longer than the clip is one ramp
    for period, n in ((0.05, 4099), ([0.05, 0.5], 7937), (1.25, 4099)):
        chain = [{"kind": "gain_envelope", "period": period, "floor": 0.25}]
        x = unit_clip(3, n)
        z = LA.apply_chain([x], chain, [9], 7)[0]
        P, ph = LA.envelope_draw(LA.parse_chain(chain)[0], LA.entry_draw(9, 7, 0), 16000)
        lo, hi = LA.envelope_range(LA.parse_chain(chain)[0], 16000)
        assert lo <= P <= hi and 0 <= ph < P
        np.testing.assert_array_equal(z.numpy(), LA.gain_envelope(x, 9, 7, 0, P, ph, 0.25).numpy())
        if P > n + ph:
            g = (z / x).numpy()[x.numpy() != 0]
            d = np.diff(g)
            assert np.all(d >= -1e-9) or np.all(d <= 1e-9)               # one ramp


def test_adjoint_against_autograd():
    """Forward and adjoint are the same operator: autograd's gradient of <w, g x> is g w, and <g x, w> = <x, g w>."""
    x = unit_clip(7, 4099).requires_grad_(True)
    w = torch.linspace(-1, 1, 4099, dtype=torch.float64)
    z = LA.apply_chain(x[None], [ENV], [3], 11)[0]
    (z * w).sum().backward()
    P, ph = LA.envelope_draw(LA.parse_chain([ENV])[0], LA.entry_draw(3, 11, 0), 16000)
    gw = LA.gain_envelope(w, 3, 11, 0, P, ph, 0.0)
    np.testing.assert_array_equal(x.grad.numpy(), gw.numpy())
    a, b = float((z.detach() * w).sum()), float((x.detach() * gw).sum())
    assert abs(a - b) <= 1e-12 * max(1.0, abs(a))
    assert torch.autograd.gradcheck(lambda v: LA.apply_chain(v[None], [ENV], [3], 11)[0], (unit_clip(8, 300).requires_grad_(True),))


def test_order_with_noise_and_suppression():
    x = unit_clip(6)[None]
    noise = {"kind": "gaussian_noise", "snr_db": 10.0}
    sup = {"kind": "sample_suppression", "seconds": 0.3}
    env = dict(ENV, floor=0.25)
    e = LA.apply_chain(x, [env], [1], 0)[0]
    # behind the envelope the noise takes its sigma from the enveloped signal ...
    a = LA.apply_chain(x, [env, noise], [1], 0)[0]
    sigma = math.sqrt(float((e ** 2).mean()) / 10.0)
    np.testing.assert_allclose((a - e).numpy(), sigma * LA.normal_draws(16000, 1, 0, 1), rtol=0, atol=1e-15)
    # ... and in front of it the noise is enveloped too (the envelope is then entry 1 and draws as entry 1)
    b = LA.apply_chain(x, [noise, env], [1], 0)[0]
    nz = LA.apply_chain(x, [noise], [1], 0)[0]
    P, ph = LA.envelope_draw(LA.parse_chain([env])[0], LA.entry_draw(1, 0, 1), 16000)
    np.testing.assert_array_equal(b.numpy(), LA.gain_envelope(nz, 1, 0, 1, P, ph, 0.25).numpy())
    assert float((a - b).abs().max()) > 1e-3
    # a suppression commutes with it in value, each entry drawing by its own index
    c = LA.apply_chain(x, [sup, env], [1], 0)[0]
    start = LA.suppression_start(LA.entry_draw(1, 0, 0)[1], 16000, 4800)
    assert int((c[start:start + 4800] != 0).sum()) == 0 and int((c == 0).sum()) == 4800
    keep = np.ones(16000, dtype=bool)
    keep[start:start + 4800] = False
    np.testing.assert_array_equal(c.numpy()[keep], LA.gain_envelope(x[0], 1, 0, 1, P, ph, 0.25).numpy()[keep])
    # two envelopes multiply
    d = LA.apply_chain(x, [env, env], [1], 0)[0]
    np.testing.assert_array_equal(d.numpy(), LA.gain_envelope(e, 1, 0, 1, P, ph, 0.25).numpy())


def test_probability_and_draws():
    x = unit_clip(4)[None]
    for step in range(5):
        np.testing.assert_array_equal(LA.apply_chain(x, [dict(ENV, prob=0.0)], [9], step).numpy(), x.numpy())
        assert not torch.equal(LA.apply_chain(x, [dict(ENV, prob=1.0)], [9], step), x)
    fired = sum(int(not torch.equal(LA.apply_chain(x, [dict(ENV, prob=0.75)], [2], s), x)) for s in range(400))
    assert 0.68 * 400 < fired < 0.82 * 400, fired           # 0.75 +- 3 sigma of 400 draws
    # the draws differ between steps, clips and entry indices; the same triple gives the same draw
    def curve(seed, step, j):
        P, ph = LA.envelope_draw(LA.parse_chain(AWARE_CHAIN)[0], LA.entry_draw(seed, step, j), 16000)
        return (P, ph), LA.envelope_curve(16000, seed, step, j, P, ph, 0.0).astype(np.float64)
    base = curve(0, 0, 0)
    assert curve(0, 0, 0)[0] == base[0] and np.array_equal(curve(0, 0, 0)[1], base[1])
    for other in (curve(0, 1, 0), curve(1, 0, 0), curve(0, 0, 1)):
        assert other[0] != base[0] and float(np.abs(other[1] - base[1]).max()) > 0.2
    # a fixed period: the gains themselves differ
    g = [LA.envelope_gains(s, t, j, 64, 0.0).astype(np.float64) for s, t, j in ((0, 0, 0), (0, 1, 0), (1, 0, 0), (0, 0, 1))]
    for other in g[1:]:
        assert abs(np.corrcoef(g[0], other)[0, 1]) < 0.5
    assert len({LA.envelope_draw(LA.parse_chain(AWARE_CHAIN)[0], LA.entry_draw(0, s, 0), 16000)[0] for s in range(32)}) > 24


# ---- 2. parsing -----------------------------------------------------------------------------------------------------------------------
def test_parse_defaults_tables_and_device_entries():
    assert list(LA.KINDS)[:8] == EIGHT and list(LA.KINDS.values()) == list(range(len(LA.KINDS)))      # the recorded table stays what it was
    assert LA.KINDS["gain_envelope"] == 8 and list(LA.KINDS)[8] == "gain_envelope"
    assert [LA.kind_id(k) for k in EIGHT + ["gain_envelope", "reverb", None]] == list(range(9)) + [None, None]
    assert "gain_envelope" not in LA.SPLITTING
    c = LA.parse_chain([{"kind": "gain_envelope", "period": 0.25}])
    assert c == [{"kind": "gain_envelope", "prob": 1.0, "period": [0.25, 0.25], "floor": 0.0}]
    assert LA.parse_chain(c) == c
    c = LA.parse_chain([{"kind": "gain_envelope", "period": (0.05, 0.5), "floor": 0.25, "prob": 0.75}])
    assert c == [{"kind": "gain_envelope", "prob": 0.75, "period": [0.05, 0.5], "floor": 0.25}]
    assert LA.envelope_range(c[0], 16000) == (800, 8000)
    assert LA.device_entries_ex(c, 16000) == [(8, 0.75, [800.0, 8000.0, 0.25, 0.0])]
    assert LA.device_mixture(LA.parse_mixture([{"weight": 0.5, "chain": c}]), 16000) == [(0.5, [(8, 0.75, [800.0, 8000.0, 0.25, 0.0])])]
    assert LA.parse_chain([{"kind": "gain_envelope", "period": 64 / 16000}])[0]["period"] == [0.004, 0.004]
    assert LA.envelope_range({"period": [0.004, 65.536]}, 16000) == (64, 1 << 20)
    LA.check_lengths(c, 16000, [256, 15872])                               # no rule: a period longer than the clip is valid
    four = LA.parse_chain([ENV] * 4)
    assert len(four) == 4 and [e[0] for e in LA.device_entries_ex(four, 16000)] == [8] * 4
    with pytest.raises(ValueError, match="at most 4"):
        LA.parse_chain([ENV] * 5)


@pytest.mark.parametrize("entry,match", [
    ({"kind": "gain_envelope"}, "period is required"),
    ({"kind": "gain_envelope", "period": 63.9 / 16000}, "outside 64"),                    # below 64 samples
    ({"kind": "gain_envelope", "period": [0.5, 0.05]}, "lo <= hi"),
    ({"kind": "gain_envelope", "period": [0.05, 65.537]}, "outside 64"),                  # above 2^20 samples
    ({"kind": "gain_envelope", "period": 0.0}, "0 < lo"),
    ({"kind": "gain_envelope", "period": [0.05, float("inf")]}, "finite"),
    ({"kind": "gain_envelope", "period": float("nan")}, "finite"),
    ({"kind": "gain_envelope", "period": [0.05, 0.1, 0.2]}, "neither a number"),
    ({"kind": "gain_envelope", "period": "slow"}, "neither a number"),
    ({"kind": "gain_envelope", "period": 0.05, "floor": 1.0}, "floor"),
    ({"kind": "gain_envelope", "period": 0.05, "floor": -0.01}, "floor"),
    ({"kind": "gain_envelope", "period": 0.05, "floor": float("nan")}, "floor"),
    ({"kind": "gain_envelope", "period": 0.05, "prob": 1.5}, "prob"),
    ({"kind": "gain_envelope", "period": 0.05, "seconds": 0.3}, r"unknown key\(s\) \['seconds'\]"),
    ({"kind": "gain_envelopes", "period": 0.05}, "unknown kind"),
])
def test_refusals(entry, match):
    with pytest.raises(ValueError, match=match):
        LA.parse_chain([entry])
    with pytest.raises(ValueError):
        LA.parse_mixture([{"weight": 0.5, "chain": [entry]}])
    from aware_amd.embedding import AWAREEmbedder
    with pytest.raises(ValueError):
        AWAREEmbedder(loss="push_extremes", verbose=False, loop_attacks=[entry])


def test_accepted_beside_every_splitting_kind():
    """In front of, behind and on both sides of every splitting kind (the message table's valid entries), beside the
    stretch-speed pair, and in every chain of a mixture; the split rule between the others is untouched."""
    table = _golden("loop_chain_messages.json")
    assert list(table["entries"]) == EIGHT
    for kind in LA.SPLITTING[:6]:
        s = table["entries"][kind]
        for chain in ([ENV, s], [s, ENV], [ENV, s, ENV], [ENV, ENV, s, ENV]):
            parsed = LA.parse_chain(chain)
            assert [a["kind"] for a in parsed] == [a["kind"] for a in chain]
            assert [e[0] for e in LA.device_entries_ex(parsed, 16000)] == [LA.kind_id(a["kind"]) for a in chain]
    LA.parse_chain([ENV, table["entries"]["time_stretch"], table["entries"]["speed_change"], ENV])
    with pytest.raises(ValueError, match="follows it directly"):
        LA.parse_chain([table["entries"]["time_stretch"], ENV, table["entries"]["speed_change"]])
    with pytest.raises(ValueError, match="not both"):
        LA.parse_chain([table["entries"]["reverberation"], ENV, table["entries"]["delete_samples"]])
    LA.parse_mixture([{"weight": 0.3, "chain": [ENV, table["entries"][k]]} for k in ("reverberation", "phase_vocoder", "delete_samples")])


def test_card_keys_reach_the_embedder(tmp_path):
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        card = yaml.safe_load(f)
    assert "loop_attacks" not in card and "loop_attack_mixture" not in card              # the committed card keeps its behaviour
    card["loop_attacks"] = yaml.safe_load("[{kind: gain_envelope, period: [0.05, 0.5], prob: 0.75}, {kind: gaussian_noise, snr_db: 20.0}]")
    card["loop_attack_seed"] = 5
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.loop_attacks == [{"kind": "gain_envelope", "prob": 0.75, "period": [0.05, 0.5], "floor": 0.0},
                                {"kind": "gaussian_noise", "prob": 1.0, "snr_db": 20.0}]
    assert emb.loop_attack_seed == 5
    del card["loop_attacks"]
    card["loop_attack_mixture"] = [{"weight": 0.5, "chain": [{"kind": "gain_envelope", "period": 0.25, "floor": 0.1}]},
                                   {"weight": 0.5, "chain": [{"kind": "sample_suppression", "seconds": 0.3}]}]
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.loop_attack_mixture[0] == {"weight": 0.5, "chain": [{"kind": "gain_envelope", "prob": 1.0, "period": [0.25, 0.25], "floor": 0.1}]}
    del card["loop_attack_mixture"]
    card["loop_attacks"] = [{"kind": "gain_envelope", "period": 0.001}]
    p.write_text(yaml.safe_dump(card))
    assert load(str(p)) is None                               # a stage that fails is reported as None, as everywhere in load()


def test_abi_symbols_and_bad_arguments():
    from aware_amd import _lib, attacks as A
    lib = _lib.load_library()
    assert "aware_gain_envelope" in _lib.SIGNATURES and hasattr(lib, "aware_gain_envelope")
    assert "loop_gain_kernels.hip" in _lib.SOURCES and len(_lib.SIGNATURES["aware_gain_envelope"][1]) == 14
    with open(os.path.join(ROOT, "include", "aware_hip.h")) as f:
        hdr = f.read()
    assert "#define AWARE_LOOP_GAIN_ENVELOPE 8" in hdr and "int aware_gain_envelope(const float* in, const int* off" in hdr
    ent = (_lib.LoopAttackEx * 1)(_lib.LoopAttackEx(8, 0.75, (C.c_float * 4)(800.0, 8000.0, 0.0, 0.0)))
    seeds = (C.c_uint32 * 1)(0)
    assert lib.aware_embed_set_loop_attacks_ex(None, ent, 1, seeds, None, 0, None) == -1
    old = (_lib.LoopAttack * 1)(_lib.LoopAttack(8, 800.0, 1.0))
    assert lib.aware_embed_set_loop_attacks(None, old, 1, seeds, None, 0, None) == -1
    # the stand-alone entry refuses null pointers and parameters out of range before anything touches a device
    p = C.c_void_p(256)                                      # never dereferenced: every call below is refused
    good = dict(B=1, max_len=16000, step=0, entry=0, p_lo=64, p_hi=800, floor=0.0)

    def call(ptrs=(p, p, p, p, p), gains=None, **kw):
        a = dict(good, **kw)
        return lib.aware_gain_envelope(ptrs[0], ptrs[1], ptrs[2], a["B"], a["max_len"], ptrs[3], a["step"], a["entry"], a["p_lo"],
                                       a["p_hi"], a["floor"], ptrs[4], gains, None)

    for i in range(5):                                       # each pointer in turn; the gains may be null
        ptrs = [p] * 5
        ptrs[i] = None
        assert call(ptrs) == -1, i
    for kw in (dict(B=0), dict(B=65536), dict(max_len=0), dict(max_len=(1 << 30) + 1), dict(step=-1), dict(entry=-1), dict(entry=4),
               dict(p_lo=63), dict(p_lo=801), dict(p_hi=(1 << 20) + 1), dict(floor=1.0), dict(floor=-0.5), dict(floor=float("nan"))):
        assert call(**kw) == -1, kw
    assert {"GainEnvelope", "Fade", "Tremolo"} <= set(A.ATTACKS)
    assert [type(a).__name__ for a in A.config3_attack_stack()] == ["Resample", "LowPassFilter", "GaussianNoise", "PCMBitDepthConversion"]
    assert len(A.reference_attack_list()) == 13
    with pytest.raises(ValueError):
        A.Fade()
    with pytest.raises(ValueError):
        A.Tremolo(4.0, 1.5)
    g = A.Fade(seconds_in=None).gain(5, 16000, "cpu")
    np.testing.assert_allclose(g.numpy(), [0.0, 0.2, 0.4, 0.6, 0.8])
    g = A.Fade(seconds_out=None).gain(5, 16000, "cpu")
    np.testing.assert_allclose(g.numpy(), [0.8, 0.6, 0.4, 0.2, 0.0])
    g = A.Fade(seconds_in=2 / 16000, seconds_out=1 / 16000).gain(6, 16000, "cpu")
    np.testing.assert_allclose(g.numpy(), [0.0, 0.5, 1.0, 1.0, 1.0, 0.0])
    t = np.arange(16000) / 16000.0
    np.testing.assert_allclose(A.Tremolo(4.0, 0.9).gain(16000, 16000, "cpu").numpy(), 1 - 0.45 * (1 + np.sin(2 * np.pi * 4.0 * t)), atol=1e-6)


def test_c_parser_on_the_cpu():
    """csrc/loop_chain.hpp through tests/host_sim/loop_chain_check (built without HIP): rc 0 exactly where parse_chain accepts,
    -1 for each bad parameter and through the older entry point; the byte count of a chain with the kind is that of the same
    chain with a noise entry in its place, so a chain that holds only the kind carves what a noise-only chain carves."""
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
    EV, NO = (8, 0.75, [800.0, 8000.0, 0.25]), one["gaussian_noise"]
    for ws in fixture["workspace"]:
        dims = _dims_case(ws["dims"])
        # accepted: alone, four of them, beside every kind in either position, around the pair; each with the bytes of its noise twin
        chains = [[EV], [EV] * 4, [EV, NO], [NO, EV]]
        for k in EIGHT[1:]:
            chains += [[EV, one[k]], [one[k], EV], [EV, one[k], EV]]
        chains.append([EV, one["time_stretch"], one["speed_change"], EV])
        twins = [[NO if e is EV else e for e in c] for c in chains]
        got = run(dims + "".join(_chain_case(c) for c in chains) + "".join(_chain_case(c) for c in twins))
        for c, (rc, nbytes), (rc2, nbytes2) in zip(chains, got[:len(chains)], got[len(chains):]):
            assert rc == 0 and rc2 == 0 and nbytes == nbytes2 > 0, (c, rc, nbytes, nbytes2)
        assert got[0][1] == ws["bytes"]["noise"]                                    # the recorded count of a noise-only chain
        # periods at the limits
        ok = [(8, 1.0, [64.0, 64.0, 0.0]), (8, 1.0, [64.0, 1048576.0, 0.0]), (8, 0.0, [1048576.0, 1048576.0, 0.999])]
        assert [rc for rc, _ in run(dims + "".join(_chain_case([e]) for e in ok))] == [0, 0, 0]
        # refused: every bad parameter, a fifth entry, and the older entry point
        nan, inf = float("nan"), float("inf")
        bad = [(8, 1.0, [63.0, 800.0, 0.0]), (8, 1.0, [800.0, 799.0, 0.0]), (8, 1.0, [800.0, 1048577.0, 0.0]), (8, 1.0, [800.5, 900.0, 0.0]),
               (8, 1.0, [800.0, 900.5, 0.0]), (8, 1.0, [nan, 800.0, 0.0]), (8, 1.0, [800.0, inf, 0.0]), (8, 1.0, [800.0, 8000.0, 1.0]),
               (8, 1.0, [800.0, 8000.0, -0.01]), (8, 1.0, [800.0, 8000.0, nan]), (8, 1.5, [800.0, 8000.0, 0.0]), (8, nan, [800.0, 8000.0, 0.0]),
               (9, 1.0, [800.0, 8000.0, 0.0])]
        assert [rc for rc, _ in run(dims + "".join(_chain_case([e]) for e in bad))] == [-1] * len(bad)
        assert run(dims + _chain_case([EV] * 5))[0] == (-1, 0)
        assert [rc for rc, _ in run(dims + _chain_case([EV], ex=0) + _chain_case([NO, EV], ex=0))] == [-1, -1]
        # the one-split rule reads past the kind: two splitting entries stay refused with an envelope between them
        assert run(dims + _chain_case([one["reverberation"], EV, one["delete_samples"]]))[0][0] == -1
        assert run(dims + _chain_case([one["time_stretch"], EV, one["speed_change"]]))[0][0] == -1


# ---- 3. the value claim, on the CPU ---------------------------------------------------------------------------------------------------
def envelope_attacks(y):
    """The six attacks of the claim on y [4, n] float32: linear fade-in and fade-out over the whole clip, tremolo at 1, 4 and 20 Hz
    with depth 0.9, the middle half ducked to 0.1.  None of them is the loop's own model."""
    n = y.shape[-1]
    t = np.arange(n, dtype=np.float64)
    out = {"fade-in": t / n, "fade-out": (n - 1 - t) / n}
    for hz in (1.0, 4.0, 20.0):
        out[f"tremolo {hz:g} Hz"] = 1.0 - 0.45 * (1.0 + np.sin(2.0 * np.pi * hz * t / 16000.0))
    duck = np.ones(n)
    duck[n // 4: n - n // 4] = 0.1
    out["middle half ducked"] = duck
    return {k: (y.astype(np.float64) * g).astype(np.float32) for k, g in out.items()}


def snr_db(audio, y):
    """Mean SNR in dB of the embeddings y (unit peak, as the loop leaves them) against their hosts at unit peak."""
    out = []
    for a, v in zip(audio, y):
        h = a[:y.shape[-1]].astype(np.float64)
        h = h / (np.abs(h).max() + 1e-8)
        out.append(10.0 * np.log10(np.sum(h ** 2) / np.sum((v.astype(np.float64) - h) ** 2)))
    return float(np.mean(out))


def test_envelope_in_the_loop_survives_moving_gains(value_setup):
    """Four 1 s clips, 400 steps, seeds 0..3: BER under six gain attacks the loop's model does not contain (fade-in and fade-out
    over the whole clip, tremolo 1 / 4 / 20 Hz at depth 0.9, the middle half ducked to 0.1) of the plain embedding and of the
    embedding with gain_envelope(period 0.05-0.5 s, floor 0, prob 0.75) inside the loop.  Clean 0 % for both, the plain mean at
    least 10 %, the aware mean at most half of it.  Measured with this restatement: plain 28.75 / 30 / 37.5 / 33.75 / 30 / 42.5 %,
    mean 33.75 %; aware 0 / 0 / 1.25 / 3.75 / 12.5 / 3.75 %, mean 3.54 %; clean 0 % for both; SNR 15.8 against 14.4 dB."""
    plain, audio, bits, wm, y0 = value_setup
    y1 = AttackedEmbedder(AWARE_CHAIN, [0, 1, 2, 3]).embed(audio, wm)[0].numpy()
    clean0, clean1 = ber(plain, bits, y0), ber(plain, bits, y1)
    a0, a1 = envelope_attacks(y0), envelope_attacks(y1)
    b0 = {k: ber(plain, bits, v) for k, v in a0.items()}
    b1 = {k: ber(plain, bits, v) for k, v in a1.items()}
    for k in b0:
        print(f"{k:20s} plain {b0[k]:6.2f} %   envelope-aware {b1[k]:6.2f} %")
    m0, m1 = float(np.mean(list(b0.values()))), float(np.mean(list(b1.values())))
    print(f"clean BER plain {clean0:.2f} % / envelope-aware {clean1:.2f} %; mean over the six: plain {m0:.2f} % / aware {m1:.2f} %; "
          f"SNR against the host: plain {snr_db(audio, y0):.1f} dB / aware {snr_db(audio, y1):.1f} dB")
    assert clean0 == 0.0 and clean1 == 0.0
    assert m0 >= 10.0
    assert m1 <= 0.5 * m0
