"""Sample deletion inside the embed loop (EXTENSION, chain kind 7): the torch restatement (aware_amd/embedding/loop_attacks.py:
delete_range, delete_count, delete_draw, delete_samples, apply_chain) against plain numpy slicing and the oracle's Cropout /
DeleteSamples, the gather-form adjoint against autograd, the validation of the entry, the card keys, the C ABI's symbols, and the
value claim on the CPU -- what a deletion at the clip's start inside the loop buys against trimming, through the oracle's embed
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
from test_loop_speed_host import snr_db

CROP = {"kind": "delete_samples", "seconds": 0.032}
ANY = {"kind": "delete_samples", "seconds": [0.01, 0.2], "at": "anywhere"}
NOISE10 = {"kind": "gaussian_noise", "snr_db": 10.0}
SUP = {"kind": "sample_suppression", "seconds": 0.3}
SPLITTERS = [{"kind": "reverberation", "rt60": 0.3}, {"kind": "speed_change", "cents": 200.0}, {"kind": "time_stretch", "rate": 1.1},
             {"kind": "pitch_shift", "cents": 100.0}, {"kind": "phase_vocoder", "rate": 1.1}]


def cut(x, start, k):
    """The definition in numpy: slice, concatenate, zeros behind."""
    return np.concatenate([x[:start], x[start + k:], np.zeros(k, dtype=x.dtype)])


# ---- 1. the model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4099, 7937])
def test_delete_samples_is_the_definition(n):
    x = unit_clip(3, n)
    for start, k in ((0, 1), (0, 513), (1001, 777), (n - 300, 300), (0, n - 1), (n - 1, 1), (0, n)):
        z = LA.delete_samples(x, start, k)
        assert z.dtype == torch.float64 and z.shape == (n,)
        np.testing.assert_array_equal(z.numpy(), cut(x.numpy(), start, k))
        assert np.all(z.numpy()[n - k:] == 0.0)
        z32 = LA.delete_samples(x.float(), start, k)
        assert z32.dtype == torch.float32
        np.testing.assert_array_equal(z32.numpy(), cut(x.float().numpy(), start, k))
    assert LA.delete_samples(x, 5, 0) is x                                                 # k = 0: the identity path
    xb = torch.stack([x, -2 * x])                                                          # the operator acts on the last axis
    np.testing.assert_array_equal(LA.delete_samples(xb, 17, 300)[1].numpy(), -2 * cut(x.numpy(), 17, 300))
    for start, k in ((-1, 5), (0, n + 1), (n - 3, 4)):
        with pytest.raises(ValueError):
            LA.delete_samples(x, start, k)


def test_at_start_is_cropout_and_anywhere_is_delete_samples():
    a, _ = make_clip(2, 16000)
    x = torch.from_numpy(a)[None]
    for step in (0, 1, 399):
        r = LA.entry_draw(5, step, 0)
        k = LA.delete_count(r[2], 1, 512)
        z = LA.apply_chain(x, [CROP], [5], step)[0].numpy()
        ref = O.cropout_attack(a, (k + 0.5) / 16000.0)                                # int() of it is k
        assert len(ref) == 16000 - k
        np.testing.assert_array_equal(z, np.concatenate([ref, np.zeros(k, dtype=np.float32)]))
        e = LA.parse_chain([ANY])[0]
        start, k = LA.delete_draw(e, r, 16000, 16000)
        assert 160 <= k <= 3200 and 0 <= start <= 16000 - k - 1 and start == LA.suppression_start(r[1], 16000, k)
        z = LA.apply_chain(x, [ANY], [5], step)[0].numpy()
        ref = O.delete_samples_attack(a, (k + 0.5) / 16000.0, start)
        assert len(ref) == 16000 - k
        np.testing.assert_array_equal(z, np.concatenate([ref, np.zeros(k, dtype=np.float32)]))


@pytest.mark.parametrize("start,k", [(0, 1), (0, 513), (311, 97), (1231, 300), (0, 1530), (77, 0)])
def test_gather_adjoint_is_autograd(start, k):
    """gx[i] = gz[i] for i < start, 0 inside the cut, gz[i - k] behind it: bit for bit what autograd gives."""
    n = 1531
    x = unit_clip(7, n).requires_grad_(True)
    gz = torch.from_numpy(np.cos(0.37 * np.arange(n)) * np.linspace(0.2, 1.0, n))
    (LA.delete_samples(x, start, k) * gz).sum().backward()
    gx = LA.delete_samples_adjoint(gz, start, k).numpy()
    loop = np.array([gz[i] if i < start else (0.0 if i < start + k else gz[i - k]) for i in range(n)])
    np.testing.assert_array_equal(gx, loop)
    np.testing.assert_array_equal(x.grad.numpy(), gx)


def test_probability_and_identity():
    x = unit_clip(4)[None]
    for step in range(5):
        np.testing.assert_array_equal(LA.apply_chain(x, [dict(CROP, prob=0.0)], [9], step).numpy(), x.numpy())
        np.testing.assert_array_equal(LA.apply_chain(x, [dict(ANY, prob=0.0)], [9], step).numpy(), x.numpy())
    fired = sum(int(not torch.equal(LA.apply_chain(x[:, :2048], [dict(CROP, prob=0.75)], [2], s), x[:, :2048])) for s in range(400))
    assert 0.68 * 400 < fired < 0.82 * 400, fired                                         # 0.75 +- 3 sigma of 400 draws


def test_order_with_noise_and_suppression():
    x = unit_clip(6)[None]
    e = LA.parse_chain([{"kind": "delete_samples", "seconds": [0.4, 0.5], "at": "anywhere"}])[0]      # a long run of zeros at the end
    start, k = LA.delete_draw(e, LA.entry_draw(1, 0, 0), 16000, 16000)
    res = LA.apply_chain(x, [e], [1], 0)[0]
    np.testing.assert_array_equal(res.numpy(), cut(x[0].numpy(), start, k))
    # noise behind the deletion: its sigma comes from the shortened signal
    both = LA.apply_chain(x, [e, NOISE10], [1], 0)[0]
    sigma = np.sqrt(float((res ** 2).mean()) / 10.0)
    np.testing.assert_allclose((both - res).numpy(), sigma * LA.normal_draws(16000, 1, 0, 1), atol=1e-12)
    # noise in front: it is cut with the clip (the draw is entry 1's)
    front = LA.apply_chain(x, [NOISE10, e], [1], 0)[0]
    noisy = LA.apply_chain(x, [NOISE10], [1], 0)[0]
    s1, k1 = LA.delete_draw(e, LA.entry_draw(1, 0, 1), 16000, 16000)
    np.testing.assert_array_equal(front.numpy(), cut(noisy.numpy(), s1, k1))
    # a suppression behind it is where it was drawn
    b = LA.apply_chain(x, [e, SUP], [1], 0)[0]
    s_b = LA.suppression_start(LA.entry_draw(1, 0, 1)[1], 16000, 4800)
    assert float(b[s_b:s_b + 4800].abs().max()) == 0.0


def test_ragged_lists():
    clips = [unit_clip(1, 7937), unit_clip(2, 40000)]
    out = LA.apply_chain(clips, [ANY], [4, 5], 2)
    assert isinstance(out, list) and [len(o) for o in out] == [7937, 40000]
    np.testing.assert_array_equal(out[1].numpy(), LA.apply_chain(clips[1][None], [ANY], [5], 2)[0].numpy())


# ---- 2. the draws ---------------------------------------------------------------------------------------------------------------
def test_draws_cover_both_ends_and_differ_between_steps_and_clips():
    assert LA.delete_count(0, 1, 512) == 1 and LA.delete_count(0xFFFFFFFF, 1, 512) == 512
    assert LA.delete_count(12345, 77, 77) == 77
    got = [LA.delete_count(LA.entry_draw(5, s, 0)[2], 3, 10) for s in range(400)]
    assert set(got) == set(range(3, 11))
    assert LA.suppression_start(0, 16000, 512) == 0 and LA.suppression_start(0xFFFFFFFF, 16000, 512) == 16000 - 512 - 1
    assert LA.suppression_start(0xFFFFFFFF, 16000, 15999) == 0                             # the longest cut starts at 0
    e = LA.parse_chain([ANY])[0]
    draws = {(sd, s): LA.delete_draw(e, LA.entry_draw(sd, s, 0), 16000, 16000) for sd in range(4) for s in range(8)}
    assert len({d[0] for d in draws.values()}) >= 30 and len({d[1] for d in draws.values()}) >= 30      # 32 draws each
    assert all(0 <= st and 160 <= k <= 3200 and st + k < 16000 for st, k in draws.values())
    x = torch.stack([unit_clip(1), unit_clip(1)])
    z0, z1 = LA.apply_chain(x, [ANY], [0, 1], 0), LA.apply_chain(x, [ANY], [0, 1], 1)
    assert not torch.equal(z0[0], z0[1]) and not torch.equal(z0[0], z1[0])
    np.testing.assert_array_equal(LA.apply_chain(x, [ANY], [0, 1], 0).numpy(), z0.numpy())         # reproducible
    np.testing.assert_array_equal(z0[1].numpy(), cut(x[1].numpy(), *draws[(1, 0)]))
    # at: start never moves the cut
    c = LA.parse_chain([CROP])[0]
    assert all(LA.delete_draw(c, LA.entry_draw(sd, s, 0), 16000, 16000)[0] == 0 for sd in range(4) for s in range(8))


# ---- 3. parsing -----------------------------------------------------------------------------------------------------------------
def test_parse_fills_defaults():
    assert LA.KINDS["delete_samples"] == 7 and LA.DELETE_AT == {"start": 0, "anywhere": 1}
    c = LA.parse_chain([{"kind": "sample_suppression", "seconds": 0.5}, {"kind": "delete_samples", "seconds": 0.032},
                        {"kind": "gaussian_noise", "snr_db": 10}])
    assert c == [{"kind": "sample_suppression", "prob": 1.0, "seconds": 0.5},
                 {"kind": "delete_samples", "prob": 1.0, "seconds": 0.032, "at": "start"},
                 {"kind": "gaussian_noise", "prob": 1.0, "snr_db": 10.0}]
    assert LA.parse_chain(c) == c                                                          # a parsed chain parses to itself
    assert LA.delete_range(c[1], 16000) == (1, 512)
    assert LA.device_entries_ex(c, 16000) == [(1, 1.0, [8000.0, 0.0, 0.0, 0.0]), (7, 1.0, [1.0, 512.0, 0.0, 0.0]),
                                              (0, 1.0, [10.0, 0.0, 0.0, 0.0])]
    r = LA.parse_chain([{"kind": "delete_samples", "seconds": (0.01, 0.2), "at": "anywhere", "prob": 0.75}])
    assert r == [{"kind": "delete_samples", "prob": 0.75, "seconds": [0.01, 0.2], "at": "anywhere"}]
    assert LA.parse_chain(r) == r
    assert LA.delete_range(r[0], 16000) == (160, 3200)
    assert LA.device_entries_ex(r, 16000) == [(7, 0.75, [160.0, 3200.0, 1.0, 0.0])]
    LA.check_lengths(c, 16000, [15872])
    LA.check_lengths(r, 16000, [3201])
    with pytest.raises(ValueError, match="clip 1"):
        LA.check_lengths(r, 16000, [8000, 3200])                                           # k_hi < Ny for every clip
    with pytest.raises(ValueError):
        LA.check_lengths(LA.parse_chain([{"kind": "delete_samples", "seconds": 0.00005}]), 16000, [16000])      # k_hi = 0
    with pytest.raises(ValueError):
        LA.check_lengths(LA.parse_chain([{"kind": "delete_samples", "seconds": [0.00005, 0.1]}]), 16000, [16000])      # k_lo = 0
    with pytest.raises(ValueError):
        LA.apply_chain(unit_clip(1, 400)[None], [CROP], [0], 0)                            # 512 >= 400
    # chains of the older kinds say what they said
    old = LA.parse_chain([{"kind": "reverberation", "rt60": 0.3}, {"kind": "gaussian_noise", "snr_db": 10}])
    assert old == [{"kind": "reverberation", "prob": 1.0, "rt60": [0.3, 0.3], "drr_db": -3.0},
                   {"kind": "gaussian_noise", "prob": 1.0, "snr_db": 10.0}]
    assert LA.device_entries_ex(old, 16000) == [(2, 1.0, [4800.0, 4800.0, -3.0, 0.0]), (0, 1.0, [10.0, 0.0, 0.0, 0.0])]
    sp = LA.parse_chain([{"kind": "time_stretch", "rate": 1.1}, {"kind": "speed_change", "cents": 200.0}])
    assert [e["kind"] for e in sp] == ["time_stretch", "speed_change"]
    assert LA.device_entries_ex(LA.parse_chain([{"kind": "speed_change", "cents": 200.0}]), 16000) == [(3, 1.0, [-7150.0, 8025.0, 0.0, 0.0])]
    assert LA.device_entries(LA.parse_chain([SUP, NOISE10]), 16000) == [(1, 4800.0, 1.0), (0, 10.0, 1.0)]


@pytest.mark.parametrize("chain", [
    [{"kind": "delete"}],
    [{"kind": "delete_samples"}],
    [{"kind": "delete_samples", "prob": 0.5}],
    [{"kind": "delete_samples", "seconds": 0.0}],
    [{"kind": "delete_samples", "seconds": -0.1}],
    [{"kind": "delete_samples", "seconds": float("nan")}],
    [{"kind": "delete_samples", "seconds": float("inf")}],
    [{"kind": "delete_samples", "seconds": [0.2, 0.1]}],
    [{"kind": "delete_samples", "seconds": [0.0, 0.1]}],
    [{"kind": "delete_samples", "seconds": [float("nan"), 0.1]}],
    [{"kind": "delete_samples", "seconds": [0.01, 0.02, 0.03]}],
    [{"kind": "delete_samples", "seconds": [0.01]}],
    [{"kind": "delete_samples", "seconds": "short"}],
    [{"kind": "delete_samples", "seconds": 0.032, "at": "end"}],
    [{"kind": "delete_samples", "seconds": 0.032, "at": 1}],
    [{"kind": "delete_samples", "seconds": 0.032, "prob": 1.5}],
    [{"kind": "delete_samples", "seconds": 0.032, "snr_db": 10.0}],
    [{"kind": "delete_samples", "seconds": 0.032, "cents": 100.0}],
    [{"kind": "delete_samples", "seconds": 0.032, "rate": 1.1}],
    [CROP, CROP],
    [CROP, NOISE10, ANY],
    [CROP, NOISE10, SUP, NOISE10, SUP],
] + [[CROP, s] for s in SPLITTERS] + [[s, CROP] for s in SPLITTERS] + [[s, NOISE10, ANY] for s in SPLITTERS]
  + [[ANY, NOISE10, s] for s in SPLITTERS])
def test_invalid_chains_are_refused(chain):
    with pytest.raises(ValueError):
        LA.parse_chain(chain)
    from aware_amd.embedding import AWAREEmbedder
    with pytest.raises(ValueError):
        AWAREEmbedder(loss="push_extremes", verbose=False, loop_attacks=chain)


def test_elementwise_entries_may_surround_it():
    c = LA.parse_chain([SUP, NOISE10, ANY, NOISE10])
    assert [e["kind"] for e in c] == ["sample_suppression", "gaussian_noise", "delete_samples", "gaussian_noise"]
    from aware_amd.embedding import AWAREEmbedder
    assert AWAREEmbedder(loss="push_extremes", verbose=False, loop_attacks=[SUP, CROP, NOISE10]).loop_attacks == LA.parse_chain([SUP, CROP, NOISE10])


# ---- 4. card and surface --------------------------------------------------------------------------------------------------------
def test_card_keys_reach_the_embedder(tmp_path):
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        text = f.read()
    assert "# loop_attacks: [{kind: delete_samples, seconds: 0.032, at: start, prob: 0.75}]" in text
    card = yaml.safe_load(text)
    assert "loop_attacks" not in card and "sync_search" not in card                        # the committed card keeps its behaviour
    card["loop_attacks"] = yaml.safe_load("[{kind: gaussian_noise, snr_db: 20.0}, {kind: delete_samples, seconds: 0.032, at: start, prob: 0.75}]")
    card["loop_attack_seed"] = 5
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.loop_attacks == [{"kind": "gaussian_noise", "prob": 1.0, "snr_db": 20.0},
                                {"kind": "delete_samples", "prob": 0.75, "seconds": 0.032, "at": "start"}]
    assert emb.loop_attack_seed == 5
    card["loop_attacks"] = [{"kind": "delete_samples", "seconds": [0.01, 0.2], "at": "anywhere"}]
    p.write_text(yaml.safe_dump(card))
    assert load(str(p))[0].loop_attacks == [{"kind": "delete_samples", "prob": 1.0, "seconds": [0.01, 0.2], "at": "anywhere"}]
    card["loop_attacks"] = [{"kind": "delete_samples", "seconds": 0.032}, {"kind": "speed_change", "cents": 200.0}]
    p.write_text(yaml.safe_dump(card))
    assert load(str(p)) is None


def test_abi_symbols_and_bad_arguments():
    from aware_amd import _lib
    lib = _lib.load_library()
    assert "aware_delete_samples" in _lib.SIGNATURES and hasattr(lib, "aware_delete_samples")
    assert "loop_delete_kernels.hip" in _lib.SOURCES
    assert len(_lib.SIGNATURES["aware_delete_samples"][1]) == 10
    assert lib.aware_version() == 350
    assert C.sizeof(_lib.LoopAttackEx) == 24 and C.sizeof(_lib.LoopAttack) == 12
    with open(os.path.join(ROOT, "include", "aware_hip.h")) as f:
        hdr = f.read()
    assert "#define AWARE_LOOP_DELETE_SAMPLES 7" in hdr and "int aware_delete_samples(const float* in, const int* off" in hdr
    ent = (_lib.LoopAttackEx * 1)(_lib.LoopAttackEx(7, 0.75, (C.c_float * 4)(1.0, 512.0, 0.0, 0.0)))
    seeds = (C.c_uint32 * 1)(0)
    assert lib.aware_embed_set_loop_attacks_ex(None, ent, 1, seeds, None, 0, None) == -1
    assert lib.aware_embed_loop_attack_workspace_bytes_ex(None, ent, 1) == 0
    old = (_lib.LoopAttack * 1)(_lib.LoopAttack(7, 512.0, 1.0))
    assert lib.aware_embed_set_loop_attacks(None, old, 1, seeds, None, 0, None) == -1
    # the stand-alone entry refuses null pointers, sizes out of range and aliasing before anything touches a device
    assert lib.aware_delete_samples(None, None, None, 1, 16000, None, None, None, 0, None) == -1
    p = C.c_void_p(256)                                     # never dereferenced: every call below is refused
    q = C.c_void_p(512)
    for i in range(6):                                      # each pointer in turn
        a = [p, p, p, p, p, q]
        a[i] = None
        assert lib.aware_delete_samples(a[0], a[1], a[2], 1, 16000, a[3], a[4], a[5], 0, None) == -1, i
    for B, max_len, adjoint in ((0, 16000, 0), (65536, 16000, 0), (-1, 16000, 0), (1, 0, 0), (1, (1 << 30) + 1, 0), (1, 16000, 2),
                                (1, 16000, -1)):
        assert lib.aware_delete_samples(p, p, p, B, max_len, p, p, q, adjoint, None) == -1, (B, max_len, adjoint)
    assert lib.aware_delete_samples(p, p, p, 1, 16000, p, p, p, 0, None) == -1             # out == in


# ---- 5. the value claim, on the CPU ---------------------------------------------------------------------------------------------
AWARE_CHAIN = [{"kind": "delete_samples", "seconds": 0.032, "prob": 0.75}]
CROPS = [192, 224, 256, 288, 320]
DELETIONS = [(k, s) for k in (800, 1728, 2400) for s in (0, 1000)]


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


def trim_table(plain, bits, y):
    """BER % after plain slicing: the crops, then the deletions."""
    crops = [ber(plain, bits, y[:, d:]) for d in CROPS]
    dels = [ber(plain, bits, np.concatenate([y[:, :s], y[:, s + k:]], axis=1)) for k, s in DELETIONS]
    return crops, dels


def test_deletion_in_the_loop_survives_trimming(value_setup):
    """Four 1 s clips, 400 steps, delete_samples(1..512 samples at the start, prob 0.75) inside the loop against plain slicing:
    the first d samples dropped, d in 192..320, and k samples cut out at s, k in {800, 1728, 2400}, s in {0, 1000}.  Bounds: clean
    0 % both, the plain means at least 10 % each, the aware means at most half of them.  Measured with this restatement: see
    DESIGN.md section 21."""
    plain, audio, bits, y0, y1 = value_setup
    clean0, clean1 = ber(plain, bits, y0), ber(plain, bits, y1)
    print(f"clean BER plain {clean0:.2f} % / deletion-aware {clean1:.2f} %")
    c0, d0 = trim_table(plain, bits, y0)
    c1, d1 = trim_table(plain, bits, y1)
    for d, b0, b1 in zip(CROPS, c0, c1):
        print(f"first {d} samples dropped: plain {b0:.2f} % / deletion-aware {b1:.2f} %")
    for (k, s), b0, b1 in zip(DELETIONS, d0, d1):
        print(f"{k} samples cut out at {s}: plain {b0:.2f} % / deletion-aware {b1:.2f} %")
    mc0, mc1, md0, md1 = float(np.mean(c0)), float(np.mean(c1)), float(np.mean(d0)), float(np.mean(d1))
    print(f"mean over the crops: plain {mc0:.2f} % / deletion-aware {mc1:.2f} %; over the deletions: plain {md0:.2f} % / "
          f"deletion-aware {md1:.2f} %")
    print("SNR against the normalised host, dB: plain " + ", ".join(f"{v:.2f}" for v in snr_db(y0, audio))
          + " / deletion-aware " + ", ".join(f"{v:.2f}" for v in snr_db(y1, audio)))
    assert clean0 == 0.0 and clean1 == 0.0
    assert mc0 >= 10.0 and md0 >= 10.0
    assert mc1 <= 0.5 * mc0
    assert md1 <= 0.5 * md0
