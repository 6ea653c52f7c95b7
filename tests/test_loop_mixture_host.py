"""Attack mixtures (EXTENSION), host side: parse_mixture, the selection rule mixture_choice, the torch
restatement apply_mixture, the card key and the ABI, and the value claim on the CPU oracle."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, make_clip
from oracle import aware_oracle as O
from aware_amd.embedding import loop_attacks as LA
from test_loop_attacks_host import AttackedEmbedder, ber, ber_half_zeroed, ber_noise5
from test_loop_delete_host import CROPS
from test_loop_reverb_host import ber_rooms
from test_loop_stretch_host import CENTS, RATES, ber_pitch, ber_stretch

MIX = [
    {"weight": 0.2, "chain": [{"kind": "sample_suppression", "seconds": 0.3, "prob": 0.75},
                              {"kind": "gaussian_noise", "snr_db": 10.0}]},
    {"weight": 0.2, "chain": [{"kind": "reverberation", "rt60": [0.1, 0.5], "drr_db": -3.0, "prob": 0.75},
                              {"kind": "gaussian_noise", "snr_db": 20.0}]},
    {"weight": 0.2, "chain": [{"kind": "phase_vocoder", "rate": [0.85, 1.15], "cents": 150.0, "prob": 0.9}]},
    {"weight": 0.2, "chain": [{"kind": "delete_samples", "seconds": [0.01, 0.2], "at": "anywhere", "prob": 0.75},
                              {"kind": "gaussian_noise", "snr_db": 10.0}]},
]  # 0.2 clean
# the remaining kernels, and no clean share
MIX2 = [
    {"weight": 0.4, "chain": [{"kind": "time_stretch", "rate": [0.85, 1.15]}, {"kind": "speed_change", "cents": 200.0}]},
    {"weight": 0.3, "chain": [{"kind": "pitch_shift", "cents": 150.0}]},
    {"weight": 0.3, "chain": [{"kind": "speed_change", "cents": 200.0}, {"kind": "gaussian_noise", "snr_db": 10.0}]},
]
NOISE = {"kind": "gaussian_noise", "snr_db": 10.0}


# ---- 1. parse_mixture -------------------------------------------------------------------------------------------------------------
def test_parse_fills_defaults():
    assert LA.parse_mixture(None) == [] and LA.parse_mixture([]) == []
    m = LA.parse_mixture([{"chain": [NOISE]}, {"chain": [{"kind": "delete_samples", "seconds": 0.032}]}])
    assert [e["weight"] for e in m] == [0.5, 0.5]                       # 1 / len: no clean share unless one is asked for
    assert m[0]["chain"] == LA.parse_chain([NOISE]) and m[1]["chain"] == LA.parse_chain([{"kind": "delete_samples", "seconds": 0.032}])
    m = LA.parse_mixture(MIX)
    assert [e["weight"] for e in m] == [0.2] * 4 and [e["chain"] for e in m] == [LA.parse_chain(e["chain"]) for e in MIX]
    assert LA.parse_mixture(MIX2)[0]["chain"][0]["prob"] == 1.0
    assert LA.parse_mixture([{"weight": 0.0, "chain": [NOISE]}])[0]["weight"] == 0.0
    eight = [{"weight": 0.125, "chain": [NOISE]}] * 8
    assert len(LA.parse_mixture(eight)) == 8
    dm = LA.device_mixture(LA.parse_mixture(MIX), 16000)
    assert [w for w, _ in dm] == [0.2] * 4 and dm[2][1] == LA.device_entries_ex(LA.parse_chain(MIX[2]["chain"]), 16000)


@pytest.mark.parametrize("mixture, index", [
    ({"weight": 1.0, "chain": [NOISE]}, None),                                           # not a list
    ([{"weight": 0.1, "chain": [NOISE]}] * 9, None),                                     # more than eight chains
    ([{"weight": 0.5, "chain": [NOISE]}, [NOISE]], 1),                                   # an entry that is no dict
    ([{"weight": 0.5, "chain": [NOISE], "prob": 1.0}], 0),                               # an unknown key
    ([{"weight": 0.5, "chain": [NOISE]}, {"weight": 0.5, "chain": []}], 1),              # an empty chain
    ([{"weight": 0.5, "chain": [NOISE]}, {"weight": 0.5}], 1),
    ([{"weight": -0.1, "chain": [NOISE]}], 0),
    ([{"weight": 0.5, "chain": [NOISE]}, {"weight": float("nan"), "chain": [NOISE]}], 1),
    ([{"weight": float("inf"), "chain": [NOISE]}], 0),
    ([{"weight": "much", "chain": [NOISE]}], 0),
    ([{"weight": 0.6, "chain": [NOISE]}, {"weight": 0.5, "chain": [NOISE]}], None),      # a sum above 1
    ([{"weight": 0.5, "chain": [NOISE]}, {"weight": 0.5, "chain": [{"kind": "reverb"}]}], 1),
    # every refusal inside one chain stays a refusal
    ([{"weight": 0.3, "chain": [NOISE]}, {"weight": 0.3, "chain": [NOISE]},
      {"weight": 0.3, "chain": [{"kind": "delete_samples", "seconds": 0.032}, {"kind": "speed_change", "cents": 200.0}]}], 2),
    ([{"weight": 0.5, "chain": [{"kind": "reverberation", "rt60": 0.3}, {"kind": "phase_vocoder", "rate": 1.1}]}], 0),
    ([{"weight": 0.5, "chain": [NOISE] * 5}], 0),
    # one set of impulse responses per handle: a second reverberation chain is refused
    ([{"weight": 0.5, "chain": [{"kind": "reverberation", "rt60": 0.3}]}, {"weight": 0.5, "chain": [{"kind": "reverberation", "rt60": 0.2}]}], 1),
])
def test_invalid_mixtures_are_refused(mixture, index):
    with pytest.raises(ValueError, match="loop_attack_mixture" + (rf"\[{index}\]" if index is not None else "")):
        LA.parse_mixture(mixture)


def test_weight_sum_tolerance():
    LA.parse_mixture([{"weight": 0.5, "chain": [NOISE]}, {"weight": 0.5 + 5e-7, "chain": [NOISE]}])
    with pytest.raises(ValueError):
        LA.parse_mixture([{"weight": 0.5, "chain": [NOISE]}, {"weight": 0.5 + 1e-5, "chain": [NOISE]}])


# ---- 2. mixture_choice ------------------------------------------------------------------------------------------------------------
def r0(seed, step):
    return int(LA.philox4x32(np.array([[0, step, 12, 1]], dtype=np.uint64), (seed, 0x5EED))[0][0])


def test_thresholds_at_float32_weights():
    w = [0.2, 0.2, 0.2, 0.2]
    acc, want = 0.0, []
    for x in w:
        acc += float(np.float32(x))                                     # float32 values, summed in double
        want.append(int(np.floor(acc * 2.0 ** 32)))
    assert LA.mixture_thresholds(w) == want
    assert want[0] == 858993472 != int(0.2 * 2 ** 32)                   # float32(0.2) > 0.2: the threshold says which one is meant
    assert LA.mixture_thresholds([1.0]) == [1 << 32] and LA.mixture_thresholds([0.5, 0.5 + 5e-7]) == [1 << 31, 1 << 32]
    assert LA.mixture_thresholds([0.0, 0.25]) == [0, 1 << 30]
    for seed, step in ((0, 0), (7, 3), (4095, 399)):
        r = r0(seed, step)
        want_c = next((c for c, t in enumerate(want) if r < t), -1)
        assert LA.mixture_choice(seed, step, w) == want_c


def test_the_draw_is_word_12():
    # the entries draw from words 1..4, the noise from word 0, the responses from word 8: word 12 is the mixture's own
    assert all(r0(5, 9) != int(LA.entry_draw(5, 9, j)[0]) for j in range(4))
    assert int(LA.philox4x32(np.array([[0, 9, 12, 1]], dtype=np.uint64), (5, 0x5EED))[0][0]) == r0(5, 9)


def test_choice_statistics_and_edge_weights():
    seeds = range(4096)
    got = np.array([LA.mixture_choice(s, 5, [0.2] * 4) for s in seeds])
    counts = [int((got == c).sum()) for c in (-1, 0, 1, 2, 3)]
    assert counts == [843, 824, 815, 860, 754]                          # the issue's figures with the host Philox twin
    draws = {step: [r0(s, step) for s in seeds] for step in (0, 399)}
    for w in ([0.2] * 4, [0.4, 0.3, 0.3], [0.1, 0.0, 0.6], [0.05] * 8):
        thr = LA.mixture_thresholds(w)
        assert list(LA.mixture_choices(range(64), 399, w)) == [LA.mixture_choice(s, 399, w) for s in range(64)]
        for step in (0, 399):
            got = np.array([next((c for c, t in enumerate(thr) if r < t), -1) for r in draws[step]])
            shares = {-1: 1.0 - float(np.sum(np.asarray(w, dtype=np.float32).astype(np.float64)))}
            shares.update({c: float(np.float32(x)) for c, x in enumerate(w)})
            for c, p in shares.items():
                n, sd = int((got == c).sum()), np.sqrt(4096 * max(p, 0.0) * (1.0 - max(p, 0.0)))
                if p < 1e-6:
                    assert n == 0, (w, step, c)                         # a zero weight is never drawn; no clean share at a sum of 1
                else:
                    assert abs(n - 4096 * p) <= 5 * sd, (w, step, c, n)
    assert all(LA.mixture_choice(s, 3, [1.0]) == 0 for s in range(256))
    got = LA.mixture_choices(seeds, 3, [0.25])
    assert set(got) == {-1, 0} and abs(int((got == -1).sum()) - 3072) <= 5 * np.sqrt(4096 * 0.75 * 0.25)


def test_choice_differs_between_steps_and_clips():
    w = [0.2] * 4
    by_step = [[LA.mixture_choice(s, step, w) for s in range(16)] for step in range(8)]
    assert len({tuple(r) for r in by_step}) == 8                        # no two steps alike
    assert all(len(set(r)) > 1 for r in by_step)                        # and no step at which all clips agree
    assert len({tuple(r[s] for r in by_step) for s in range(16)}) == 16


# ---- 3. apply_mixture -------------------------------------------------------------------------------------------------------------
def unit(seed, n):
    x = torch.from_numpy(np.random.default_rng(seed).standard_normal(n))
    return x / x.abs().max()


@pytest.mark.parametrize("mixture", [MIX, MIX2], ids=["four_families", "tempo_pitch"])
def test_apply_mixture_is_apply_chain_of_the_choice(mixture):
    w = [m["weight"] for m in mixture]
    seeds = list(range(100, 112))
    x = torch.stack([unit(s, 8192) for s in seeds])
    seen = set()
    for step in (0, 7):
        z = LA.apply_mixture(x, mixture, seeds, step)
        assert torch.is_tensor(z) and z.shape == x.shape
        for b, s in enumerate(seeds):
            c = LA.mixture_choice(s, step, w)
            seen.add(c)
            ref = x[b] if c < 0 else LA.apply_chain(x[b][None], mixture[c]["chain"], [s], step)[0]
            assert torch.equal(z[b], ref), (step, b, c)
    assert seen == set(range(len(mixture))) | ({-1} if sum(w) < 0.99 else set())


def test_apply_mixture_ragged_and_autograd():
    w = [m["weight"] for m in MIX]
    seeds = [108, 109, 110, 111, 113, 117]                              # choices 3, -1, 2, 2, 0, 1 at step 0
    assert [LA.mixture_choice(s, 0, w) for s in seeds] == [3, -1, 2, 2, 0, 1]
    xs = [unit(s, n).requires_grad_(True) for s, n in zip(seeds, (8192, 6144, 7936, 5120, 9000, 8448))]
    zs = LA.apply_mixture(xs, MIX, seeds, 0)
    assert isinstance(zs, list) and [len(z) for z in zs] == [len(x) for x in xs]
    assert zs[1] is xs[1]                                               # choice -1 is the identity
    gs = [unit(1000 + s, len(x)) for s, x in zip(seeds, xs)]
    sum((z * g).sum() for z, g in zip(zs, gs)).backward()
    for b, s in enumerate(seeds):
        c = LA.mixture_choice(s, 0, w)
        x2 = xs[b].detach().clone().requires_grad_(True)
        z2 = x2 if c < 0 else LA.apply_chain([x2], MIX[c]["chain"], [s], 0)[0]
        (z2 * gs[b]).sum().backward()
        assert torch.equal(zs[b].detach(), z2.detach()) and torch.equal(xs[b].grad, x2.grad), (b, c)
    short = [{"weight": 0.5, "chain": [NOISE]}, {"weight": 0.5, "chain": [{"kind": "sample_suppression", "seconds": 0.3}]}]
    with pytest.raises(ValueError, match=r"loop_attack_mixture\[1\].*clip 1"):
        LA.apply_mixture([torch.zeros(8000), torch.zeros(3000)], short, [0, 1], 0)     # check_lengths runs per chain
    with pytest.raises(ValueError, match="2 clips but 1 seeds"):
        LA.apply_mixture(torch.zeros(2, 8000), MIX, [0], 0)


# ---- 4. card and ABI --------------------------------------------------------------------------------------------------------------
def test_card_key_reaches_the_embedder(tmp_path):
    from aware_amd.embedding import AWAREEmbedder
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        text = f.read()
    assert "# loop_attack_mixture: [{weight: " in text
    card = yaml.safe_load(text)
    assert "loop_attack_mixture" not in card and "loop_attacks" not in card            # the committed card keeps its behaviour
    assert load()[0].loop_attack_mixture == []
    card["loop_attack_mixture"] = yaml.safe_load(yaml.safe_dump(MIX))
    card["loop_attack_seed"] = 9
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.loop_attack_mixture == LA.parse_mixture(MIX) and emb.loop_attacks == [] and emb.loop_attack_seed == 9
    card["loop_attacks"] = [NOISE]                                      # both keys: the embedder raises, load() reports None
    p.write_text(yaml.safe_dump(card))
    assert load(str(p)) is None
    with pytest.raises(ValueError, match="not both"):
        AWAREEmbedder(loss="push_extremes", loop_attacks=[NOISE], loop_attack_mixture=MIX, verbose=False)
    del card["loop_attacks"]
    card["loop_attack_mixture"] = [{"weight": 0.7, "chain": [NOISE]}, {"weight": 0.7, "chain": [NOISE]}]
    p.write_text(yaml.safe_dump(card))
    assert load(str(p)) is None


def test_abi_symbols_and_bad_arguments():
    from aware_amd import _lib
    lib = _lib.load_library()
    for name in ("aware_embed_loop_mixture_workspace_bytes", "aware_embed_set_loop_mixture", "aware_loop_mixture_draw"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "loop_mix_kernels.hip" in _lib.SOURCES
    assert lib.aware_version() == 350                                   # added without a version step
    assert C.sizeof(_lib.LoopChain) == 16
    with open(os.path.join(ROOT, "include", "aware_hip.h")) as f:
        hdr = f.read()
    assert "typedef struct aware_loop_chain { const aware_loop_attack_ex* attacks; int n_attacks; float weight; } aware_loop_chain;" in hdr
    assert "size_t aware_embed_loop_mixture_workspace_bytes(const aware_batch*" in hdr
    assert "int aware_embed_set_loop_mixture(aware_embed* e, const aware_loop_chain* chains, int n_chains" in hdr
    assert "int aware_loop_mixture_draw(const uint32_t* seeds, int B, int step, const float* weights, int n_chains" in hdr
    ent = (_lib.LoopAttackEx * 1)(_lib.LoopAttackEx(0, 1.0, (C.c_float * 4)(10.0, 0.0, 0.0, 0.0)))
    chains = (_lib.LoopChain * 1)(_lib.LoopChain(C.cast(ent, C.POINTER(_lib.LoopAttackEx)), 1, 1.0))
    seeds = (C.c_uint32 * 1)(0)
    # refused before anything touches a device
    assert lib.aware_embed_set_loop_mixture(None, chains, 1, seeds, None, 0, None) == -1
    assert lib.aware_embed_loop_mixture_workspace_bytes(None, chains, 1) == 0
    w = (C.c_float * 2)(0.5, 0.5)
    p = C.c_void_p(256)                                                 # never dereferenced: every call below is refused
    assert lib.aware_loop_mixture_draw(None, 4, 0, w, 2, p, None) == -1
    assert lib.aware_loop_mixture_draw(p, 4, 0, None, 2, p, None) == -1
    assert lib.aware_loop_mixture_draw(p, 4, 0, w, 2, None, None) == -1
    assert lib.aware_loop_mixture_draw(p, 0, 0, w, 2, p, None) == -1
    assert lib.aware_loop_mixture_draw(p, 4, 0, w, 0, p, None) == -1 and lib.aware_loop_mixture_draw(p, 4, 0, w, 9, p, None) == -1
    for bad in ((0.6, 0.5), (-0.1, 0.5), (float("nan"), 0.5), (float("inf"), 0.0)):
        assert lib.aware_loop_mixture_draw(p, 4, 0, (C.c_float * 2)(*bad), 2, p, None) == -1, bad


# ---- 5. the value claim, on the CPU -------------------------------------------------------------------------------------------------
class MixtureEmbedder(AttackedEmbedder):
    """The oracle's loop with the mixture between its two normalisers."""

    def recompute_magnitude(self, mag_full, phase):
        y = O.istft(mag_full * torch.exp(1j * phase))
        y = y / torch.amax(torch.abs(y) + 1e-8, dim=-1, keepdim=True)
        y = LA.apply_mixture(y, self.chain, self.seeds, self.step)
        self.step += 1
        y = y / torch.amax(torch.abs(y) + 1e-8, dim=-1, keepdim=True)
        return torch.abs(O.stft(y)), y


FAMILIES = ("noise at 5 dB", "half the clip zeroed", "rooms of rt60 0.3 s", "phase-vocoder TimeStretch", "PitchShift", "first samples dropped")
# the families on which the mixture also meets the project's bar for a single kind, at most half of plain, with 2.5 points to spare
HALF_OF_PLAIN = ("noise at 5 dB", "rooms of rt60 0.3 s", "phase-vocoder TimeStretch", "first samples dropped")


def family_table(plain, bits, y):
    """Mean BER % per family at the evaluation points of the single-kind host tests, with their own evaluators."""
    return {"noise at 5 dB": ber_noise5(plain, bits, y),
            "half the clip zeroed": ber_half_zeroed(plain, bits, y),
            "rooms of rt60 0.3 s": ber_rooms(plain, bits, y),
            "phase-vocoder TimeStretch": float(np.mean([ber_stretch(plain, bits, y, r) for r in RATES])),
            "PitchShift": float(np.mean([ber_pitch(plain, bits, y, c) for c in CENTS])),
            "first samples dropped": float(np.mean([ber(plain, bits, y[:, d:]) for d in CROPS]))}


def test_one_mixture_against_six_families():
    """Four 1 s clips, seeds 0..3, 400 steps on the CPU oracle: the plain watermark and one embedded under MIX, both evaluated
    under noise at 5 dB, half the clip zeroed, fixed rooms of rt60 0.3 s, the oracle's phase-vocoder TimeStretch at 0.9..1.1 and
    PitchShift at +-50 / +-100 cents, and the first 192..320 samples dropped.  Hard conditions: clean BER 0 % for both, and on
    every family the mixture's mean at least 5 points (4 bit errors of 80) below the plain watermark's of the same run.  The
    project's bar for a single kind, at most half of plain, is asserted where the measured figure meets it with 2.5 points to
    spare (HALF_OF_PLAIN).  Measured, plain / mixture, 400 steps: noise 22.97 / 2.34, zeroed 38.96 / 21.88, rooms 42.08 / 14.58,
    TimeStretch 31.88 / 8.75, PitchShift 51.88 / 46.88, dropped 23.50 / 0.75 %.
    The mixture's limitation: it MISSES half of plain on `half the clip zeroed` (21.88 against 19.48: the loop zeroes 0.3 s, a
    fifth of the steps) and on `PitchShift` (46.88 against 25.94: the gain is the 5 points the hard condition asks for and no
    more; the vocoder's pitch mode is drawn at one step in ten).  DESIGN.md section 22 has the table and the longer runs."""
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    pairs = [make_clip(s, 16000) for s in range(4)]
    audio = np.stack([p[0] for p in pairs])
    bits = np.stack([p[1] for p in pairs])
    wm = np.stack([O.bits_to_bipolar(b) for b in bits]).astype(np.float32)
    plain = O.Embedder()
    y0 = plain.embed(audio, wm)[0].numpy()
    y1 = MixtureEmbedder(MIX, [0, 1, 2, 3]).embed(audio, wm)[0].numpy()
    clean0, clean1 = ber(plain, bits, y0), ber(plain, bits, y1)
    print(f"clean BER plain {clean0:.2f} % / mixture {clean1:.2f} %")
    t0, t1 = family_table(plain, bits, y0), family_table(plain, bits, y1)
    for k in FAMILIES:
        print(f"{k}: plain {t0[k]:.2f} % / mixture {t1[k]:.2f} %")
    assert clean0 == 0.0 and clean1 == 0.0
    for k in FAMILIES:
        assert t1[k] <= t0[k] - 5.0, (k, t0[k], t1[k])
    for k in HALF_OF_PLAIN:
        assert t1[k] <= 0.5 * t0[k], (k, t0[k], t1[k])
