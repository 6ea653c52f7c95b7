"""Attack-aware embedding (EXTENSION): the torch restatement of the loop's attack chain (aware_amd/embedding/loop_attacks.py)
against the oracle's post-hoc attacks, the validation of the chain, the card keys, and the value claim on the CPU -- what an
attack inside the loop buys, through the oracle's embed loop.  No GPU."""
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, make_clip
from oracle import aware_oracle as O
from aware_amd.embedding import loop_attacks as LA

NOISE10 = [{"kind": "gaussian_noise", "snr_db": 10.0}]


def unit_clip(seed, n=16000, dtype=torch.float64):
    a, _ = make_clip(seed, n)
    x = torch.from_numpy(a).to(dtype)
    return x / (x.abs().max() + 1e-8)


# ---- 1. ties of the restatement ---------------------------------------------------------------------------------------------
def test_philox_matches_the_oracles():
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, size=(257, 4), dtype=np.uint64).astype(np.uint32)
    for key in ((0, 0x5EED), (7, 0x5EED), (0xFFFFFFFF, 0xDEADBEEF)):
        np.testing.assert_array_equal(LA.philox4x32(ctr, key), O.philox4x32(ctr, key))


@pytest.mark.parametrize("seed,snr", [(0, 10.0), (3, 5.0), (123456, 20.0)])
def test_noise_at_step_0_is_the_post_hoc_attack(seed, snr):
    a, _ = make_clip(seed + 10, 16001)                      # a length that is no multiple of four
    ref = O.gaussian_noise_attack(a, snr, seed)
    chain = [{"kind": "gaussian_noise", "snr_db": snr}]
    z64 = LA.apply_chain(torch.from_numpy(a).double()[None], chain, [seed], 0)[0]
    np.testing.assert_array_equal(z64.numpy().astype(np.float32), ref)
    z32 = LA.apply_chain(torch.from_numpy(a)[None], chain, [seed], 0)[0]
    assert z32.dtype == torch.float32
    ulp = float(np.spacing(np.float32(np.abs(ref).max())))
    err = float(np.abs(z32.numpy().astype(np.float64) - ref.astype(np.float64)).max())
    print(f"float32 restatement against the oracle: max error {err:.2e}, one ulp of the peak {ulp:.2e}")
    assert err <= ulp


@pytest.mark.parametrize("seconds,n", [(0.5, 16000), (0.3, 16000), (0.25, 40000)])
def test_suppression_is_the_post_hoc_attack(seconds, n):
    a, _ = make_clip(2, n)
    k = int(seconds * 16000)
    for step in (0, 1, 399):
        r = LA.entry_draw(5, step, 0)
        start = (int(r[1]) * (n - k)) >> 32
        assert 0 <= start <= n - k - 1
        z = LA.apply_chain(torch.from_numpy(a)[None], [{"kind": "sample_suppression", "seconds": seconds}], [5], step)[0]
        np.testing.assert_array_equal(z.numpy(), O.sample_suppression_attack(a, seconds, start=start))


def test_draws_differ_between_steps_and_clips():
    x = torch.stack([unit_clip(1), unit_clip(1)])
    z0 = LA.apply_chain(x, NOISE10, [0, 1], 0)
    z1 = LA.apply_chain(x, NOISE10, [0, 1], 1)
    e00, e01, e10 = (z0[0] - x[0]).numpy(), (z0[1] - x[1]).numpy(), (z1[0] - x[0]).numpy()
    for u, v in ((e00, e01), (e00, e10)):
        assert abs(np.corrcoef(u, v)[0, 1]) < 0.05
    # the same seed and step give the same draw
    np.testing.assert_array_equal(LA.apply_chain(x, NOISE10, [0, 1], 0).numpy(), z0.numpy())
    starts = {LA.suppression_start(LA.entry_draw(0, s, 0)[1], 16000, 4800) for s in range(32)}
    assert len(starts) > 24
    # a second noise entry of the same chain draws its own noise
    two = LA.apply_chain(x[:1], NOISE10 + NOISE10, [0], 0)[0]
    one = LA.apply_chain(x[:1], NOISE10, [0], 0)[0]
    assert abs(np.corrcoef((two - one).numpy(), (one - x[0]).numpy())[0, 1]) < 0.05


def test_noise_amplitude_and_probability():
    x = unit_clip(4)[None]
    z = LA.apply_chain(x, NOISE10, [9], 3)
    snr = 10 * np.log10(float((x ** 2).mean()) / float(((z - x) ** 2).mean()))
    assert abs(snr - 10.0) < 0.2
    chain0 = [{"kind": "gaussian_noise", "snr_db": 5.0, "prob": 0.0}, {"kind": "sample_suppression", "seconds": 0.5, "prob": 0.0}]
    for step in range(5):
        np.testing.assert_array_equal(LA.apply_chain(x, chain0, [9], step).numpy(), x.numpy())
    half = [{"kind": "sample_suppression", "seconds": 0.5, "prob": 0.75}]
    fired = sum(int((LA.apply_chain(x, half, [2], s) == 0).sum() >= 8000) for s in range(400))
    assert 0.68 * 400 < fired < 0.82 * 400, fired          # 0.75 +- 3 sigma of 400 draws


def test_chain_order_matters():
    x = unit_clip(6)[None]
    sup = {"kind": "sample_suppression", "seconds": 0.3}
    noise = {"kind": "gaussian_noise", "snr_db": 10.0}
    a = LA.apply_chain(x, [sup, noise], [1], 0)[0]
    b = LA.apply_chain(x, [noise, sup], [1], 0)[0]
    assert int((a == 0).sum()) == 0                          # the noise fills the gap
    gap = (b == 0).nonzero().flatten()
    assert len(gap) == 4800 and int(gap[-1] - gap[0]) == 4799
    start = LA.suppression_start(LA.entry_draw(1, 0, 1)[1], 16000, 4800)      # the suppression is entry 1 of the second chain
    assert int(gap[0]) == start


def test_chain_is_differentiable_with_sigma_detached():
    x = unit_clip(7, 4000).requires_grad_(True)
    chain = [{"kind": "sample_suppression", "seconds": 0.1}, {"kind": "gaussian_noise", "snr_db": 5.0}]
    z = LA.apply_chain(x[None], chain, [3], 11)[0]
    w = torch.linspace(-1, 1, 4000, dtype=torch.float64)
    (z * w).sum().backward()
    start = LA.suppression_start(LA.entry_draw(3, 11, 0)[1], 4000, 1600)
    mask = torch.ones(4000, dtype=torch.float64)
    mask[start:start + 1600] = 0
    np.testing.assert_array_equal(x.grad.numpy(), (w * mask).numpy())       # identity through the noise, the mask otherwise


def test_ragged_lists():
    clips = [unit_clip(1, 16000), unit_clip(2, 40000)]
    out = LA.apply_chain(clips, NOISE10, [4, 5], 2)
    assert isinstance(out, list) and [len(o) for o in out] == [16000, 40000]
    np.testing.assert_array_equal(out[1].numpy(), LA.apply_chain(clips[1][None], NOISE10, [5], 2)[0].numpy())


# ---- 2. validation, card keys -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [
    [{"kind": "reverb"}],
    [{"kind": "gaussian_noise", "snr_db": 10.0, "seconds": 1.0}],
    [{"kind": "gaussian_noise"}],
    [{"kind": "gaussian_noise", "snr_db": float("nan")}],
    [{"kind": "gaussian_noise", "snr_db": 10.0, "prob": 1.5}],
    [{"kind": "sample_suppression", "seconds": 0.3, "prob": -0.1}],
    [{"kind": "sample_suppression", "seconds": 0.0}],
    [{"kind": "sample_suppression", "seconds": 0.3, "start": 5}],
    [{"kind": "gaussian_noise", "snr_db": 10.0}] * 5,
    {"kind": "gaussian_noise", "snr_db": 10.0},
])
def test_invalid_chains_are_refused(chain):
    with pytest.raises(ValueError):
        LA.parse_chain(chain)
    from aware_amd.embedding import AWAREEmbedder
    with pytest.raises(ValueError):
        AWAREEmbedder(loss="push_extremes", verbose=False, loop_attacks=chain)


def test_parse_fills_defaults_and_lengths_are_checked():
    assert LA.parse_chain(None) == [] and LA.parse_chain([]) == []
    c = LA.parse_chain([{"kind": "sample_suppression", "seconds": 0.5}, {"kind": "gaussian_noise", "snr_db": 10}])
    assert c == [{"kind": "sample_suppression", "prob": 1.0, "seconds": 0.5}, {"kind": "gaussian_noise", "prob": 1.0, "snr_db": 10.0}]
    assert LA.device_entries(c, 16000) == [(1, 8000.0, 1.0), (0, 10.0, 1.0)]
    LA.check_lengths(c, 16000, [15872, 8192])
    with pytest.raises(ValueError, match="clip 1"):
        LA.check_lengths(c, 16000, [15872, 7936])
    with pytest.raises(ValueError, match="clip 0"):
        LA.apply_chain(torch.zeros(1, 8000), c, [0], 0)


def test_card_keys_reach_the_embedder(tmp_path):
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        card = yaml.safe_load(f)
    assert "loop_attacks" not in card and "loop_attack_seed" not in card      # the committed card keeps its behaviour
    plain, _ = load()
    assert plain.loop_attacks == [] and plain.loop_attack_seed == 0
    card["loop_attacks"] = [{"kind": "gaussian_noise", "snr_db": 10.0}, {"kind": "sample_suppression", "seconds": 0.3, "prob": 0.75}]
    card["loop_attack_seed"] = 17
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.loop_attacks == [{"kind": "gaussian_noise", "prob": 1.0, "snr_db": 10.0},
                                {"kind": "sample_suppression", "prob": 0.75, "seconds": 0.3}]
    assert emb.loop_attack_seed == 17
    card["loop_attacks"] = [{"kind": "reverb"}]
    p.write_text(yaml.safe_dump(card))
    assert load(str(p)) is None                               # a stage that fails is reported as None, as everywhere in load()


# ---- 3. the value claim, on the CPU -------------------------------------------------------------------------------------------
class AttackedEmbedder(O.Embedder):
    """The oracle's loop with the chain between its two normalisers; the step advances with every loop body."""

    def __init__(self, chain, seeds, **kw):
        super().__init__(**kw)
        self.chain, self.seeds, self.step = chain, seeds, 0

    def recompute_magnitude(self, mag_full, phase):
        y = O.istft(mag_full * torch.exp(1j * phase))
        y = y / torch.amax(torch.abs(y) + 1e-8, dim=-1, keepdim=True)
        y = LA.apply_chain(y, self.chain, self.seeds, self.step)
        self.step += 1
        y = y / torch.amax(torch.abs(y) + 1e-8, dim=-1, keepdim=True)
        return torch.abs(O.stft(y)), y


@pytest.fixture(scope="module")
def value_setup():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    pairs = [make_clip(s, 16000) for s in range(4)]
    audio = np.stack([p[0] for p in pairs])
    bits = np.stack([p[1] for p in pairs])
    wm = np.stack([O.bits_to_bipolar(b) for b in bits]).astype(np.float32)
    plain = O.Embedder()
    y0 = plain.embed(audio, wm)[0].numpy()
    return plain, audio, bits, wm, y0


def ber(plain, bits, z):
    return 100.0 * float((O.decode_bits(plain.detect_raw(np.asarray(z, dtype=np.float32)).numpy()) != bits).mean())


def ber_noise5(plain, bits, y):
    return float(np.mean([ber(plain, bits, np.stack([O.gaussian_noise_attack(y[b], 5.0, seed=1000 * sd + b) for b in range(4)]))
                          for sd in range(8)]))


def ber_half_zeroed(plain, bits, y):
    out = []
    for st in (0, 1500, 3000, 4500, 6000, 7800):
        z = y.copy()
        z[:, st:st + 8000] = 0
        out.append(ber(plain, bits, z))
    return float(np.mean(out))


def test_noise_in_the_loop_buys_noise_margin(value_setup):
    """Four 1 s clips, 400 steps: BER under Gaussian noise at 5 dB SNR (8 seeds per clip) of the plain embedding and of the
    embedding with noise at 10 dB inside the loop.  Measured with this restatement: 23.28 % against 0 %, both clean 0 %."""
    plain, audio, bits, wm, y0 = value_setup
    y1 = AttackedEmbedder(NOISE10, [0, 1, 2, 3]).embed(audio, wm)[0].numpy()
    clean0, clean1 = ber(plain, bits, y0), ber(plain, bits, y1)
    n0, n1 = ber_noise5(plain, bits, y0), ber_noise5(plain, bits, y1)
    print(f"clean BER plain {clean0:.2f} % / noise-aware {clean1:.2f} %; at 5 dB: plain {n0:.2f} % / noise-aware {n1:.2f} %")
    assert clean0 == 0.0 and clean1 == 0.0
    assert n0 >= 10.0
    assert n1 <= 0.5 * n0


def test_suppression_in_the_loop_survives_half_the_clip(value_setup):
    """The same clips with 0.5 s zeroed at a random place on 75 % of the steps inside the loop, against 0.5 s zeroed at six
    fixed starts.  Measured with this restatement: 38.33 % plain against 0.625 %, clean 0 %."""
    plain, audio, bits, wm, y0 = value_setup
    chain = [{"kind": "sample_suppression", "seconds": 0.5, "prob": 0.75}]
    y2 = AttackedEmbedder(chain, [0, 1, 2, 3]).embed(audio, wm)[0].numpy()
    clean0, clean2 = ber(plain, bits, y0), ber(plain, bits, y2)
    s0, s2 = ber_half_zeroed(plain, bits, y0), ber_half_zeroed(plain, bits, y2)
    print(f"clean BER plain {clean0:.2f} % / suppression-aware {clean2:.2f} %; 0.5 s zeroed: plain {s0:.2f} % / aware {s2:.2f} %")
    assert clean0 == 0.0 and clean2 == 0.0
    assert s0 >= 10.0
    assert s2 <= 0.5 * s0


# ---- the one-split rule: the messages of parse_chain, and the C parser and carver on the CPU --------------------------------
def _golden(name):
    import json
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


def test_parse_chain_messages_are_the_recorded_ones():
    """tests/golden/loop_chain_messages.json, recorded from parse_chain before the exclusion rule was stated once: every ordered
    pair of the eight kinds with valid parameters and the chains that exercise the stretch-then-speed pair, "ok" or the message."""
    table = _golden("loop_chain_messages.json")
    assert list(table["entries"]) == list(LA.KINDS)[:8] and len(table["cases"]) == 64 + 6
    for case in table["cases"]:
        chain = [table["entries"][k] for k in case["chain"]]
        try:
            LA.parse_chain(chain)
            got = "ok"
        except ValueError as err:
            got = str(err)
        assert got == case["result"], case["chain"]


def _entry_lines(entries):
    return "".join(f"{k} {pr!r} " + " ".join(repr(float(x)) for x in (list(p) + [0.0] * 4)[:4]) + "\n" for k, pr, p in entries)


def _chain_case(entries, ex=1):
    return f"chain {len(entries)} {ex}\n" + _entry_lines(entries)


def _mixture_case(chains):
    return f"mixture {len(chains)}\n" + "".join(f"{w!r} {len(e)}\n" + _entry_lines(e) for e, w in chains)


def _dims_case(d):
    return f"dims {d['B']} {d['NS']} {d['NF']} {d['pstride']} " + " ".join(str(n) for n in d["out_len"]) + "\n"


def loop_chain_check():
    """tests/host_sim/loop_chain_check.cpp, built without HIP where it is missing or older than its sources.  Returns
    run(text) -> [(return code, bytes)], one pair per case of the program's input `text`."""
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

    return run


def test_c_parser_and_carver_on_the_cpu():
    """csrc/loop_chain.hpp through tests/host_sim/loop_chain_check.cpp, built without HIP: the return code is 0 exactly where
    parse_chain accepts the chain (the message table's chains through device_entries_ex); the byte counts of the bench tool's
    variants and mixtures are those recorded on the device before the parser and the carver moved
    (tests/golden/loop_chains_sha256.json, with the batches' dimensions); the -1 / -2 cases of test_workspace_and_error_codes."""
    import importlib.util
    run = loop_chain_check()
    spec = importlib.util.spec_from_file_location("loop_attack_bench", os.path.join(ROOT, "tools", "loop_attack_bench.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    fixture = _golden("loop_chains_sha256.json")
    ragged, short = fixture["workspace"]
    assert ragged["lengths"] == [16000, 12000, 9000] and short["lengths"] == [16000, 8000]

    # 1. the message table: every entry alone through device_entries_ex, so that a chain parse_chain refuses reaches the C parser too
    table = _golden("loop_chain_messages.json")
    one = {k: LA.device_entries_ex(LA.parse_chain([a]), 16000)[0] for k, a in table["entries"].items()}
    got = run(_dims_case(ragged["dims"]) + "".join(_chain_case([one[k] for k in case["chain"]]) for case in table["cases"]))
    for case, (rc, nbytes) in zip(table["cases"], got):
        assert (rc == 0) == (case["result"] == "ok") and rc in (0, -1), (case["chain"], rc)
        assert nbytes > 0
    # ... and the older entry points refuse kinds 2 to 7
    got = run(_dims_case(ragged["dims"]) + "".join(_chain_case([one[k]], ex=0) for k in list(LA.KINDS)[:8]))
    assert [rc for rc, _ in got] == [0, 0] + [-1] * 6

    # 2. the recorded byte counts
    for ws in (ragged, short):
        names = list(ws["bytes"])
        assert len(names) == (15 if ws is ragged else 14)
        text = _dims_case(ws["dims"])
        for name in names:
            if name in tool.VARIANTS:
                text += _chain_case(LA.device_entries_ex(LA.parse_chain(tool.VARIANTS[name]), 16000))
            else:
                text += _mixture_case([(e, w) for w, e in LA.device_mixture(LA.parse_mixture(tool.MIXTURES[name]), 16000)])
        for name, (rc, nbytes) in zip(names, run(text)):
            assert rc == 0 and nbytes == ws["bytes"][name], (ws["lengths"], name, rc, nbytes)

    # 3. test_workspace_and_error_codes on the batch [16000, 8000]: one chain of weight 1 is the chain's own workspace, rounded
    # up to 256, then int [B]; the refused mixtures
    B = short["dims"]["B"]
    chains = [LA.device_entries_ex(LA.parse_chain(c), 16000) for c in
              (tool.MIXTURES["four_families"][0]["chain"], tool.MIXTURES["four_families"][1]["chain"],
               tool.MIXTURES["four_families"][2]["chain"], tool.MIXTURES["tempo_pitch"][0]["chain"], tool.VARIANTS["pitch"])]
    got = run(_dims_case(short["dims"]) + "".join(_chain_case(e) + _mixture_case([(e, 1.0)]) for e in chains))
    for (rc1, ex), (rc2, mixed) in zip(got[0::2], got[1::2]):
        assert rc1 == 0 and rc2 == 0 and mixed == ((ex + 255) & ~255) + 4 * B
    NO, SU, RV = (0, 1.0, [10.0]), (1, 1.0, [4800.0]), (2, 1.0, [1600.0, 8000.0, -3.0])
    DS, SP = (7, 1.0, [1.0, 512.0, 1.0]), (3, 1.0, [-3678.0, 3896.0])
    bad = [([([NO], -0.1)], -1), ([([NO], float("nan"))], -1), ([([NO], float("inf"))], -1),
           ([([NO], 0.6), ([SU], 0.5)], -1),                            # a sum above 1
           ([([NO], 0.5), ([(9, 1.0, [0.0])], 0.5)], -1),               # what the _ex setter refuses, per chain
           ([([NO], 0.5), ([DS, SP], 0.5)], -1),                        # two kinds that split one chain
           ([([NO] * 5, 0.5)], -1),
           ([([RV], 0.5), ([RV, NO], 0.5)], -1),                        # a second reverberation chain
           ([([NO], 0.5), ([(1, 1.0, [7936.0])], 0.5)], -2)]            # k >= Ny of the 8000-sample clip
    got = run(_dims_case(short["dims"]) + "".join(_mixture_case(m) for m, _ in bad) + _mixture_case([([NO], 0.5), ([SU], 0.5 + 5e-7)]))
    for (m, want), (rc, nbytes) in zip(bad, got):
        assert rc == want and (nbytes == 0 or rc == -2), (m, rc, nbytes)
    assert got[-1][0] == 0                                               # a sum within 1 + 1e-6
