"""Reverberation inside the embed loop (EXTENSION): the torch restatement (aware_amd/embedding/loop_attacks.py: reverb_length,
reverb_ir, apply_chain) against numpy, the validation of the entry, the card keys, the C ABI's symbols, and the value claim on
the CPU -- what a reverberation inside the loop buys against fixed room responses and an echo, through the oracle's embed
loop.  No GPU."""
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

REVERB = {"kind": "reverberation", "rt60": 0.3, "drr_db": -3.0}
NOISE10 = {"kind": "gaussian_noise", "snr_db": 10.0}
SUP = {"kind": "sample_suppression", "seconds": 0.3}


def drawn(seed, step, j, entry, sr=16000):
    """(on, n_h, h) of a parsed reverberation entry at chain index j."""
    r = LA.entry_draw(seed, step, j)
    n_h = LA.reverb_length(r[2], *LA.reverb_taps(entry, sr))
    return LA.fires(r[0], entry["prob"]), n_h, LA.reverb_ir(seed, step, j, n_h, entry["drr_db"])


# ---- 1. the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny,rt60", [(7936, 0.0375), (7936, 0.128), (7936, 0.512), (15872, [0.1, 0.5]), (4001, 0.3)])
def test_apply_chain_is_the_truncated_convolution(ny, rt60):
    """z = np.convolve(x, h)[:Ny] in float64 to 1e-12 of the peak, for responses shorter and longer (8192 taps) than the clip."""
    x = unit_clip(3, ny)
    chain = LA.parse_chain([dict(REVERB, rt60=rt60)])
    for step in (0, 1, 7):
        on, n_h, h = drawn(9, step, 0, chain[0])
        assert on and len(h) == n_h
        z = LA.apply_chain(x[None], chain, [9], step)[0].numpy()
        ref = np.convolve(x.numpy(), h)[:ny]
        err = np.abs(z - ref).max() / np.abs(ref).max()
        assert err < 1e-12, (step, n_h, err)
    z32 = LA.apply_chain(x.float()[None], chain, [9], 0)[0]
    assert z32.dtype == torch.float32 and z32.shape == (ny,)
    on, n_h, h = drawn(9, 0, 0, chain[0])
    ref = np.convolve(x.numpy(), h)[:ny]
    assert np.abs(z32.numpy() - ref).max() / np.abs(ref).max() < 2e-6


def test_length_is_uniform_on_the_closed_range():
    n_lo, n_hi = 1600, 1607
    got = [LA.reverb_length(LA.entry_draw(5, s, 0)[2], n_lo, n_hi) for s in range(400)]
    assert min(got) == n_lo and max(got) == n_hi and set(got) == set(range(n_lo, n_hi + 1))
    assert LA.reverb_length(0, 2, 8192) == 2 and LA.reverb_length(0xFFFFFFFF, 2, 8192) == 8192
    assert LA.reverb_length(12345, 4800, 4800) == 4800
    wide = [LA.reverb_length(LA.entry_draw(5, s, 0)[2], 1600, 8000) for s in range(400)]
    assert 1600 <= min(wide) < 1700 and 7900 < max(wide) <= 8000       # 400 draws on 6401 values: both ends within 100
    # the restatement applies this length: the response ends where it says
    chain = LA.parse_chain([dict(REVERB, rt60=[0.1, 0.5])])
    imp = torch.zeros(1, 15872, dtype=torch.float64)
    imp[0, 0] = 1.0
    for s in range(3):
        z = LA.apply_chain(imp, chain, [5], s)[0].numpy()
        n_h = LA.reverb_length(LA.entry_draw(5, s, 0)[2], 1600, 8000)
        assert np.abs(z[n_h:]).max() < 1e-14 and abs(z[n_h - 1]) > 1e-9


@pytest.mark.parametrize("drr", [-3.0, 0.0, 6.0, -12.5])
def test_direct_to_reverberant_ratio_and_decay(drr):
    for n_h in (2, 3, 600, 4800, 8192):
        h = LA.reverb_ir(1, 4, 2, n_h, drr)
        assert len(h) == n_h and h.dtype == np.float64
        tail = float(np.sum(h[1:] ** 2))
        assert h[0] > 0 and abs(h[0] ** 2 / tail / 10.0 ** (drr / 10.0) - 1.0) < 1e-12
    # the tail is the normal draws of counter word 8 under an envelope that is 60 dB down at n_h; index 0 is discarded
    eps = LA.normal_draws(4800, 1, 4, 2, word=8)
    h = LA.reverb_ir(1, 4, 2, 4800, drr)
    np.testing.assert_allclose(h[1:], eps[1:] * np.exp(-np.log(1000.0) * np.arange(1, 4800) / 4800), rtol=1e-14)
    assert abs(np.corrcoef(eps, LA.normal_draws(4800, 1, 4, 2))[0, 1]) < 0.06            # not the noise entries' stream
    env = np.sqrt(np.convolve(h[1:] ** 2, np.ones(400) / 400, mode="valid"))
    assert 50.0 < 20 * np.log10(env[0] / env[-1]) < 60.0


def test_draws_differ_between_steps_clips_and_entries():
    e = LA.parse_chain([REVERB])[0]
    h = {k: drawn(*k, e)[2] for k in [(0, 0, 0), (0, 1, 0), (1, 0, 0), (0, 0, 1)]}
    base = h[(0, 0, 0)]
    env = np.exp(-np.log(1000.0) * np.arange(4800) / 4800)
    for k in [(0, 1, 0), (1, 0, 0), (0, 0, 1)]:
        # the normals under the envelope: 4799 independent pairs have a correlation of 0.0144 rms
        assert abs(np.corrcoef((base / env)[1:], (h[k] / env)[1:])[0, 1]) < 0.06, k
    np.testing.assert_array_equal(drawn(0, 0, 0, e)[2], base)                             # reproducible
    x = torch.stack([unit_clip(1), unit_clip(1)])
    z0, z1 = LA.apply_chain(x, [REVERB], [0, 1], 0), LA.apply_chain(x, [REVERB], [0, 1], 1)
    assert float((z0[0] - z0[1]).abs().max()) > 0.1 and float((z0[0] - z1[0]).abs().max()) > 0.1
    np.testing.assert_array_equal(LA.apply_chain(x, [REVERB], [0, 1], 0).numpy(), z0.numpy())
    # the entry's index keys the draw: behind an entry that never fires the response is another one
    shifted = LA.apply_chain(x[:1], [dict(NOISE10, prob=0.0), REVERB], [0], 0)[0]
    assert float((shifted - z0[0]).abs().max()) > 0.1
    np.testing.assert_allclose(shifted.numpy(), np.convolve(x[0].numpy(), h[(0, 0, 1)])[:16000], atol=1e-12)


def test_probability_and_identity():
    x = unit_clip(4)[None]
    off = [dict(REVERB, prob=0.0)]
    for step in range(5):
        np.testing.assert_array_equal(LA.apply_chain(x, off, [9], step).numpy(), x.numpy())
    fired = sum(int(not torch.equal(LA.apply_chain(x[:, :512], [dict(REVERB, rt60=0.01, prob=0.75)], [2], s), x[:, :512]))
                for s in range(400))
    assert 0.68 * 400 < fired < 0.82 * 400, fired                                         # 0.75 +- 3 sigma of 400 draws


def test_autograd_is_the_correlation_with_h():
    ny = 4000
    x = unit_clip(7, ny).requires_grad_(True)
    chain = LA.parse_chain([dict(REVERB, rt60=0.2)])
    z = LA.apply_chain(x[None], chain, [3], 11)[0]
    w = torch.linspace(-1, 1, ny, dtype=torch.float64) ** 3
    (z * w).sum().backward()
    _, n_h, h = drawn(3, 11, 0, chain[0])
    ref = np.correlate(np.concatenate([w.numpy(), np.zeros(n_h - 1)]), h, mode="valid")   # gx[i] = sum_k h_k gy[i + k]
    assert ref.shape == (ny,)
    assert np.abs(x.grad.numpy() - ref).max() / np.abs(ref).max() < 1e-12
    # with a mask in front and noise behind: the mask applies to the correlation, the noise is transparent
    x2 = unit_clip(7, ny).requires_grad_(True)
    z2 = LA.apply_chain(x2[None], [dict(SUP, seconds=0.1), dict(REVERB, rt60=0.2), NOISE10], [3], 11)[0]
    (z2 * w).sum().backward()
    start = LA.suppression_start(LA.entry_draw(3, 11, 0)[1], ny, 1600)
    _, n_h1, h1 = drawn(3, 11, 1, chain[0])
    ref2 = np.correlate(np.concatenate([w.numpy(), np.zeros(n_h1 - 1)]), h1, mode="valid")
    ref2[start:start + 1600] = 0
    assert np.abs(x2.grad.numpy() - ref2).max() / np.abs(ref2).max() < 1e-12


def test_ragged_lists():
    clips = [unit_clip(1, 7936), unit_clip(2, 40000)]
    out = LA.apply_chain(clips, [REVERB], [4, 5], 2)
    assert isinstance(out, list) and [len(o) for o in out] == [7936, 40000]
    np.testing.assert_array_equal(out[1].numpy(), LA.apply_chain(clips[1][None], [REVERB], [5], 2)[0].numpy())


def test_order_with_noise_and_suppression():
    x = unit_clip(6)[None]
    e = LA.parse_chain([REVERB])[0]
    # noise behind the reverberation: its sigma comes from the convolved signal
    conv = LA.apply_chain(x, [REVERB], [1], 0)[0]
    both = LA.apply_chain(x, [REVERB, NOISE10], [1], 0)[0]
    snr = 10 * np.log10(float((conv ** 2).mean()) / float(((both - conv) ** 2).mean()))
    assert abs(snr - 10.0) < 0.2
    sigma = np.sqrt(float((conv ** 2).mean()) / 10.0)
    np.testing.assert_allclose((both - conv).numpy(), sigma * LA.normal_draws(16000, 1, 0, 1), atol=1e-12)
    # noise in front: it is convolved too (the response is entry 1's)
    front = LA.apply_chain(x, [NOISE10, REVERB], [1], 0)[0]
    noisy = LA.apply_chain(x, [NOISE10], [1], 0)[0]
    np.testing.assert_allclose(front.numpy(), np.convolve(noisy.numpy(), drawn(1, 0, 1, e)[2])[:16000], atol=1e-12)
    # a suppression in front leaves the tail of what precedes it inside the gap; behind, the gap is silent
    a = LA.apply_chain(x, [SUP, REVERB], [1], 0)[0]
    b = LA.apply_chain(x, [REVERB, SUP], [1], 0)[0]
    s_a = LA.suppression_start(LA.entry_draw(1, 0, 0)[1], 16000, 4800)
    s_b = LA.suppression_start(LA.entry_draw(1, 0, 1)[1], 16000, 4800)
    assert s_a > 0 and float(a[s_a:s_a + 4800].abs().max()) > 1e-3
    assert float(b[s_b:s_b + 4800].abs().max()) == 0.0 and int((b == 0).sum()) == 4800


# ---- 2. validation, card keys, ABI ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [
    [{"kind": "reverb"}],
    [{"kind": "reverb", "rt60": 0.3}],
    [{"kind": "reverberation"}],
    [{"kind": "reverberation", "drr_db": -3.0}],
    [{"kind": "reverberation", "rt60": 0.0}],
    [{"kind": "reverberation", "rt60": -0.1}],
    [{"kind": "reverberation", "rt60": [0.5, 0.1]}],
    [{"kind": "reverberation", "rt60": [0.0, 0.1]}],
    [{"kind": "reverberation", "rt60": float("nan")}],
    [{"kind": "reverberation", "rt60": [0.1, float("inf")]}],
    [{"kind": "reverberation", "rt60": "long"}],
    [{"kind": "reverberation", "rt60": 0.3, "drr_db": float("nan")}],
    [{"kind": "reverberation", "rt60": 0.3, "drr_db": float("inf")}],
    [{"kind": "reverberation", "rt60": 0.3, "prob": 1.5}],
    [{"kind": "reverberation", "rt60": 0.3, "seconds": 0.3}],
    [{"kind": "reverberation", "rt60": 0.3, "snr_db": 10.0}],
    [{"kind": "reverberation", "rt60": 0.3}, {"kind": "reverberation", "rt60": 0.2}],
    [{"kind": "reverberation", "rt60": 0.3}, NOISE10, SUP, NOISE10, SUP],
])
def test_invalid_chains_are_refused(chain):
    with pytest.raises(ValueError):
        LA.parse_chain(chain)
    from aware_amd.embedding import AWAREEmbedder
    with pytest.raises(ValueError):
        AWAREEmbedder(loss="push_extremes", verbose=False, loop_attacks=chain)


def test_parse_fills_defaults_and_lengths_are_checked():
    assert LA.MAX_ATTACKS == 4 and LA.MAX_IR == 8192 and LA.KINDS["reverberation"] == 2
    c = LA.parse_chain([{"kind": "reverberation", "rt60": 0.3}, {"kind": "gaussian_noise", "snr_db": 10}])
    assert c == [{"kind": "reverberation", "prob": 1.0, "rt60": [0.3, 0.3], "drr_db": -3.0},
                 {"kind": "gaussian_noise", "prob": 1.0, "snr_db": 10.0}]
    assert LA.parse_chain(c) == c                                                          # a parsed chain parses to itself
    assert LA.device_entries_ex(c, 16000) == [(2, 1.0, [4800.0, 4800.0, -3.0, 0.0]), (0, 1.0, [10.0, 0.0, 0.0, 0.0])]
    r = LA.parse_chain([{"kind": "reverberation", "rt60": [0.1, 0.5], "drr_db": 2.0, "prob": 0.75}])
    assert LA.device_entries_ex(r, 16000) == [(2, 0.75, [1600.0, 8000.0, 2.0, 0.0])]
    # chains of the older kinds: device_entries is what it was, device_entries_ex says the same in the wider struct
    old = LA.parse_chain([{"kind": "sample_suppression", "seconds": 0.5}, {"kind": "gaussian_noise", "snr_db": 10}])
    assert LA.device_entries(old, 16000) == [(1, 8000.0, 1.0), (0, 10.0, 1.0)]
    assert LA.device_entries_ex(old, 16000) == [(1, 1.0, [8000.0, 0.0, 0.0, 0.0]), (0, 1.0, [10.0, 0.0, 0.0, 0.0])]
    LA.check_lengths(r, 16000, [7936])                                                    # a response longer than the clip is fine
    LA.check_lengths(LA.parse_chain([{"kind": "reverberation", "rt60": 0.512}]), 16000, [7936])      # 8192 taps
    LA.check_lengths(LA.parse_chain([{"kind": "reverberation", "rt60": 0.000125}]), 16000, [7936])   # 2 taps
    for rt60, sr in ((0.5121, 16000), (0.0001, 16000), (0.3, 44100), ([0.00005, 0.3], 16000)):
        with pytest.raises(ValueError, match="taps"):
            LA.check_lengths(LA.parse_chain([{"kind": "reverberation", "rt60": rt60}]), sr, [15872])
    with pytest.raises(ValueError, match="taps"):
        LA.apply_chain(torch.zeros(1, 8000), [{"kind": "reverberation", "rt60": 0.6}], [0], 0)


def test_card_keys_reach_the_embedder(tmp_path):
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        card = yaml.safe_load(f)
    card["loop_attacks"] = [{"kind": "reverberation", "rt60": [0.1, 0.5], "drr_db": -3.0, "prob": 0.75},
                            {"kind": "gaussian_noise", "snr_db": 10.0}]
    card["loop_attack_seed"] = 5
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.loop_attacks == [{"kind": "reverberation", "prob": 0.75, "rt60": [0.1, 0.5], "drr_db": -3.0},
                                {"kind": "gaussian_noise", "prob": 1.0, "snr_db": 10.0}]
    assert emb.loop_attack_seed == 5
    card["loop_attacks"] = [{"kind": "reverberation", "rt60": 0.3}, {"kind": "reverberation", "rt60": 0.2}]
    p.write_text(yaml.safe_dump(card))
    assert load(str(p)) is None


def test_abi_symbols_and_null_handles():
    from aware_amd import _lib
    lib = _lib.load_library()
    for name in ("aware_embed_loop_attack_workspace_bytes_ex", "aware_embed_set_loop_attacks_ex", "aware_convolve_workspace_bytes",
                 "aware_convolve", "aware_reverb_ir"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "loop_reverb_kernels.hip" in _lib.SOURCES
    assert lib.aware_version() == 350
    assert C.sizeof(_lib.LoopAttackEx) == 24 and C.sizeof(_lib.LoopAttack) == 12
    ent = (_lib.LoopAttackEx * 1)(_lib.LoopAttackEx(2, 1.0, (C.c_float * 4)(4800.0, 4800.0, -3.0, 0.0)))
    seeds = (C.c_uint32 * 1)(0)
    assert lib.aware_embed_set_loop_attacks_ex(None, ent, 1, seeds, None, 0, None) == -1
    assert lib.aware_embed_loop_attack_workspace_bytes_ex(None, ent, 1) == 0
    assert lib.aware_embed_buffer(None, 13) is None
    # the stand-alone entries refuse null pointers and sizes out of range before anything touches a device
    assert lib.aware_convolve(None, None, None, 1, 16000, None, 8192, None, 0, None, None, 0, None) == -1
    assert lib.aware_reverb_ir(None, 1, 0, 0, 4800, 4800, -3.0, None, 8192, None, None) == -1
    n = lib.aware_convolve_workspace_bytes(4, 7936, 4 * 7936, 8192)
    # the twiddles, four partition spectra and ceil(7936 / 2048) = 4 block spectra per clip, of 2056 complex values each
    assert n >= 8 * (1024 + 2056) + 8 * 2056 * 4 * (4 + 4) and n < 8 * (1024 + 2056) + 8 * 2056 * 4 * (4 + 4) + 3 * 256
    assert lib.aware_convolve_workspace_bytes(4, 7936, 4 * 7936, 600) < n                  # one partition
    for bad in ((0, 7936, 7936, 600), (4, 0, 0, 600), (4, 7936, 4 * 7936, 0), (4, 7936, 4 * 7936, 8193), (4, 7936, 7935, 600),
                (4, 7936, 4 * 7936 + 1, 600)):
        assert lib.aware_convolve_workspace_bytes(*bad) == 0, bad


def test_the_attack_is_registered():
    from aware_amd import attacks as A
    a = A.make_attack("Reverberation", rt60=0.3, drr_db=-3.0, seed=4)
    assert a.name == "reverb_0.3" and (a.rt60, a.drr_db, a.seed) == (0.3, -3.0, 4)
    assert A.Reverberation().name == "reverb_0.3"
    assert not any(isinstance(x, A.Reverberation) for x in A.reference_attack_list())
    assert not any(isinstance(x, A.Reverberation) for x in A.config3_attack_stack())


# ---- 3. the value claim, on the CPU ---------------------------------------------------------------------------------------------
AWARE_CHAIN = [{"kind": "reverberation", "rt60": [0.1, 0.5], "drr_db": -3.0, "prob": 0.75}]


def room_response(rng_seed, rt60=0.3, drr_db=-3.0, sr=16000):
    """An evaluation response of the model's shape from numpy's generator (not one the loop can have drawn)."""
    n_h = int(rt60 * sr)
    h = np.random.default_rng(rng_seed).standard_normal(n_h) * np.exp(-np.log(1000.0) * np.arange(n_h) / n_h)
    h[0] = 0.0
    h[0] = 10.0 ** (drr_db / 20.0) * np.sqrt(np.sum(h * h))
    return h


def ber_rooms(plain, bits, y):
    from scipy.signal import fftconvolve
    return float(np.mean([ber(plain, bits, np.stack([fftconvolve(c.astype(np.float64), room_response(s))[:len(c)] for c in y]))
                          for s in range(3)]))


def ber_echo(plain, bits, y, d=1600, g=0.7):
    z = y.astype(np.float64).copy()
    z[:, d:] += g * y[:, :-d]
    return ber(plain, bits, z)


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
    return plain, bits, y0, y1


def test_reverberation_in_the_loop_survives_rooms(value_setup):
    """Four 1 s clips, 400 steps, reverberation(rt60 0.1-0.5 s, -3 dB, prob 0.75) inside the loop against three fixed responses
    of rt60 0.3 s drawn from numpy's generator.  Measured with this restatement: 42.08 % plain against 8.33 %, both clean 0 %."""
    plain, bits, y0, y1 = value_setup
    clean0, clean1 = ber(plain, bits, y0), ber(plain, bits, y1)
    r0, r1 = ber_rooms(plain, bits, y0), ber_rooms(plain, bits, y1)
    print(f"clean BER plain {clean0:.2f} % / reverberation-aware {clean1:.2f} %; rt60 0.3 s: plain {r0:.2f} % / aware {r1:.2f} %")
    assert clean0 == 0.0 and clean1 == 0.0
    assert r0 >= 10.0
    assert r1 <= 0.5 * r0


def test_reverberation_in_the_loop_survives_an_echo(value_setup):
    """The same two embeddings under a single echo, y[1600:] += 0.7 y[:-1600] (100 ms).  Measured with this restatement:
    23.75 % plain against 7.50 %."""
    plain, bits, y0, y1 = value_setup
    e0, e1 = ber_echo(plain, bits, y0), ber_echo(plain, bits, y1)
    print(f"echo 100 ms x 0.7: plain {e0:.2f} % / reverberation-aware {e1:.2f} %")
    assert e0 >= 10.0
    assert e1 <= 0.5 * e0
