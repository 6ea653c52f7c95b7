"""Attack-aware embedding at any STFT geometry (keys general_geometry + general_loop_attacks), host side.

This file holds the restatement the device tests (tests/test_gpu_general_chain.py) compare against: `AttackedGeneralLoop`,
GeneralLoop with the chain between two pairs of normalisers,

    x = N(N(istft)),  z = apply_chain(x, chain, seeds, step, sample_rate),  a = N(N(z)),  |stft(a)|

the step advancing with every loop body.  Then: its tie to the card restatement (AttackedEmbedder), the keys, the value claim
at 2048 / 512 / 2048 and 44.1 kHz on the CPU, and the C parser and carver (csrc/loop_any_chain.hpp) through
tests/host_sim/general_chain_check on the CPU.  No GPU."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, make_clip
from oracle import aware_oracle as O
from aware_amd.embedding import loop_attacks as LA
from test_general_geometry_host import GeneralLoop
from test_loop_attacks_host import AttackedEmbedder

NOISE10 = {"kind": "gaussian_noise", "snr_db": 10.0}
SERVED = ("gaussian_noise", "sample_suppression", "gain_envelope")


def norm1(y):
    return y / torch.amax(torch.abs(y) + 1e-8, dim=-1, keepdim=True)


class AttackedGeneralLoop(GeneralLoop):
    """GeneralLoop with the chain in it: istft -> N -> N -> apply_chain(..., sample_rate) -> N -> N -> stft.  `step` is the
    optimiser step the next loop body draws at; it advances per loop body."""

    def __init__(self, chain, seeds, *args, step=0, **kw):
        super().__init__(*args, **kw)
        self.chain, self.seeds, self.step = LA.parse_chain(chain, self.sample_rate), list(seeds), step

    def recompute_magnitude(self, mag_full, phase):
        y = norm1(norm1(self.istft(mag_full * torch.exp(1j * phase))))
        z = LA.apply_chain(y, self.chain, self.seeds, self.step, self.sample_rate)
        self.step += 1
        a = norm1(norm1(z))
        return torch.abs(self.stft(a)), a


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [[NOISE10], [{"kind": "sample_suppression", "seconds": 0.3}, NOISE10],
                                   [{"kind": "gain_envelope", "period": [0.05, 0.5]}]])
def test_restatement_is_the_card_restatement_at_the_card_geometry(chain):
    """float64, 1024 / 256 / 1024 at 16 kHz: first-iteration loss and gradient of AttackedGeneralLoop against AttackedEmbedder's,
    1e-6 relative.  The card restatement normalises once on either side of the chain; a second normaliser moves a unit-peak
    signal by about 1e-8."""
    clips = np.stack([make_clip(s, 16000)[0] for s in (11, 12)])
    wm = np.stack([O.bits_to_bipolar(make_clip(s, 16000)[1]).astype(np.float32) for s in (11, 12)])
    out = []
    for emb in (AttackedEmbedder(LA.parse_chain(chain), [5, 7], dtype=torch.float64),
                AttackedGeneralLoop(chain, [5, 7], dtype=torch.float64)):
        with torch.no_grad():
            mag0, phase = emb.analyse(torch.from_numpy(clips).double())
        c = mag0[:, emb.band].clone().requires_grad_(True)
        loss, _ = emb.forward_loss(c, mag0, phase, torch.from_numpy(wm).double())
        loss.sum().backward()
        assert emb.step == 1
        out.append((loss.detach(), c.grad.detach()))
    (l0, g0), (l1, g1) = out
    dl = float(((l0 - l1).abs() / l0.abs()).max())
    dg = float((g0 - g1).norm() / g0.norm())
    print(f"{[a['kind'] for a in chain]}: loss {dl:.1e}, gradient rel L2 {dg:.1e} (bound 1e-6)")
    assert dl < 1e-6 and dg < 1e-6


# ---- 2. keys --------------------------------------------------------------------------------------------------------------------------
def _embedder(n_fft, hop, win, sr=16000, **kw):
    from aware_amd.embedding import AWAREEmbedder
    kw.setdefault("loss", "push_extremes")
    return AWAREEmbedder(frame_length=n_fft, hop_length=hop, win_length=win, general_geometry=True, verbose=False,
                         detection_net_cfg={"n_fft": n_fft, "sample_rate": sr}, **kw)


ONE_OF_EACH = {
    "reverberation": {"kind": "reverberation", "rt60": 0.3},
    "speed_change": {"kind": "speed_change", "cents": 100.0},
    "time_stretch": {"kind": "time_stretch", "rate": 1.1},
    "pitch_shift": {"kind": "pitch_shift", "cents": 100.0},
    "phase_vocoder": {"kind": "phase_vocoder", "rate": 1.1},
    "delete_samples": {"kind": "delete_samples", "seconds": 0.03},
    "band_filter": {"kind": "band_filter", "response": "lowpass", "freq": 3000.0},
    "excerpt": {"kind": "excerpt", "seconds": 0.5},
    "time_warp": {"kind": "time_warp", "depth": 0.04, "period": 0.128},
    "frequency_shift": {"kind": "frequency_shift", "hz": 100.0},
}


def test_both_keys_construct():
    chain = [{"kind": "gain_envelope", "period": [0.05, 0.5], "prob": 0.75}, {"kind": "sample_suppression", "seconds": 0.5},
             NOISE10, {"kind": "gain_envelope", "period": 0.05}]
    for n_fft, hop, win, sr in ((512, 128, 512, 16000), (2048, 512, 2048, 44100)):
        emb = _embedder(n_fft, hop, win, sr, general_loop_attacks=True, loop_attacks=chain)
        assert emb.general_geometry and emb.general_loop_attacks and emb.loop_attacks == LA.parse_chain(chain)


def test_load_passes_the_key_through(tmp_path):
    from aware_amd.utils.models import load
    card = tmp_path / "card.yaml"
    text = ("frame_length: 2048\nhop_length: 512\nwin_length: 2048\ngeneral_geometry: true\n"
            "detection_net_cfg: {sample_rate: 44100, n_fft: 2048}\nverbose: false\n"
            "loop_attacks: [{kind: sample_suppression, seconds: 0.5, prob: 0.75}, {kind: gaussian_noise, snr_db: 10.0}]\n")
    card.write_text(text + "general_loop_attacks: true\n")
    emb, det = load(str(card))
    assert emb.general_geometry and emb.general_loop_attacks and [a["kind"] for a in emb.loop_attacks] == ["sample_suppression", "gaussian_noise"]
    card.write_text(text)
    assert load(str(card)) is None            # the new key absent: refused at construction, which load() reports as None


def test_refusals_with_both_keys_on():
    assert set(ONE_OF_EACH) | set(SERVED) == set(LA.KINDS)
    for kind, entry in ONE_OF_EACH.items():
        with pytest.raises(NotImplementedError, match=kind) as exc:
            _embedder(512, 128, 512, general_loop_attacks=True, loop_attacks=[NOISE10, entry])
        msg = str(exc.value)
        assert "general_geometry" in msg and all(k in msg for k in SERVED), msg
    with pytest.raises(NotImplementedError, match="loop_attack_mixture") as exc:
        _embedder(512, 128, 512, general_loop_attacks=True, loop_attack_mixture=[{"weight": 0.5, "chain": [NOISE10]}])
    assert "general_geometry" in str(exc.value)
    # without the new key the refusal is the one it was, and names the key that opens the three kinds
    with pytest.raises(NotImplementedError, match="loop_attacks is not supported with general_geometry=True") as exc:
        _embedder(512, 128, 512, loop_attacks=[NOISE10])
    assert "general_loop_attacks" in str(exc.value)


def test_the_new_key_alone_changes_nothing():
    from aware_amd.embedding import AWAREEmbedder
    chain = [NOISE10, ONE_OF_EACH["speed_change"]]
    a = AWAREEmbedder(verbose=False, loss="push_extremes", loop_attacks=chain)
    b = AWAREEmbedder(verbose=False, loss="push_extremes", loop_attacks=chain, general_loop_attacks=True)
    assert not a.general_loop_attacks and b.general_loop_attacks and not b.general_geometry
    assert a.loop_attacks == b.loop_attacks == LA.parse_chain(chain)
    skip = {"general_loop_attacks", "detection_net", "loss", "audio_preprocess_pipeline", "audio_postprocess_pipeline", "_opt", "_sched"}
    assert {k: v for k, v in vars(a).items() if k not in skip} == {k: v for k, v in vars(b).items() if k not in skip}
    assert set(vars(a)) == set(vars(b))


# ---- 3. the value claim, on the CPU -----------------------------------------------------------------------------------------------------
SR, GEOM44 = 44100, (2048, 512, 2048)


@pytest.fixture(scope="module")
def setup44():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    pairs = [make_clip(s, SR) for s in range(4)]
    audio = np.stack([p[0] for p in pairs])
    bits = np.stack([p[1] for p in pairs])
    wm = np.stack([O.bits_to_bipolar(b) for b in bits]).astype(np.float32)
    plain = GeneralLoop(*GEOM44, "hann", SR)
    y0 = plain.embed(audio, wm)[0].numpy()
    return plain, audio, bits, wm, y0


def ber(loop, bits, z):
    return 100.0 * float((O.decode_bits(loop.detect_raw(np.asarray(z, dtype=np.float32)).numpy()) != bits).mean())


def noise5(y):
    """gaussian noise at 5 dB, 8 draws per clip"""
    return {f"draw {sd}": np.stack([O.gaussian_noise_attack(y[b], 5.0, seed=1000 * sd + b) for b in range(4)]) for sd in range(8)}


def half_zeroed(y):
    """Ny // 2 samples zeroed from f * Ny on"""
    ny, out = y.shape[-1], {}
    for f in (0.0, 0.1, 0.2, 0.3, 0.4, 0.49):
        z = y.copy()
        st = int(f * ny)
        z[:, st:st + ny // 2] = 0
        out[f"from {f:g} Ny"] = z
    return out


def gain_curves(y, sr=SR):
    """The six curves of tests/test_loop_gain_host.py::envelope_attacks at this sample rate: linear fade-in and fade-out over the
    whole clip, tremolo at 1, 4 and 20 Hz with depth 0.9, the middle half at 0.1."""
    n = y.shape[-1]
    t = np.arange(n, dtype=np.float64)
    out = {"fade-in": t / n, "fade-out": (n - 1 - t) / n}
    for hz in (1.0, 4.0, 20.0):
        out[f"tremolo {hz:g} Hz"] = 1.0 - 0.45 * (1.0 + np.sin(2.0 * np.pi * hz * t / sr))
    duck = np.ones(n)
    duck[n // 4: n - n // 4] = 0.1
    out["middle half at 0.1"] = duck
    return {k: (y.astype(np.float64) * g).astype(np.float32) for k, g in out.items()}


CLAIMS = {
    "noise": ([NOISE10], noise5),
    "suppression": ([{"kind": "sample_suppression", "seconds": 0.5, "prob": 0.75}], half_zeroed),
    "envelope": ([{"kind": "gain_envelope", "period": [0.05, 0.5], "floor": 0.0, "prob": 0.75}], gain_curves),
}


def claim(name, detect_ber, y0, y1):
    """The three conditions of a claim on the plain embedding y0 and the aware one y1: clean 0 % for both, the plain mean at least
    10 %, the aware mean at most half of it.  Prints every figure first."""
    attack = CLAIMS[name][1]
    clean0, clean1 = detect_ber(y0), detect_ber(y1)
    b0 = {k: detect_ber(v) for k, v in attack(y0).items()}
    b1 = {k: detect_ber(v) for k, v in attack(y1).items()}
    for k in b0:
        print(f"{name:12s} {k:20s} plain {b0[k]:6.2f} %   aware {b1[k]:6.2f} %")
    m0, m1 = float(np.mean(list(b0.values()))), float(np.mean(list(b1.values())))
    print(f"{name}: clean BER plain {clean0:.2f} % / aware {clean1:.2f} %; mean plain {m0:.2f} % / aware {m1:.2f} %")
    assert clean0 == 0.0 and clean1 == 0.0
    assert m0 >= 10.0
    assert m1 <= 0.5 * m0


@pytest.mark.parametrize("name", list(CLAIMS))
def test_a_chain_in_the_loop_buys_robustness_at_44100(setup44, name):
    """2048 / 512 / 2048 hann at 44.1 kHz, four make_clip(s, 44100) clips, 400 steps, seeds 0..3.  Measured with this restatement
    (plain mean -> aware mean): noise at 5 dB 26.56 -> 0.31 % (the Philox noise of O.gaussian_noise_attack); half the clip zeroed
    51.04 -> 0.00 % (47.5 / 50 / 51.25 / 52.5 / 52.5 / 52.5 % plain); the six gain curves 40.21 -> 2.92 % (43.75 / 38.75 / 37.5 /
    35 / 37.5 / 48.75 % plain, 1.25 / 1.25 / 0 / 2.5 / 2.5 / 10 % aware); clean 0 % everywhere."""
    plain, audio, bits, wm, y0 = setup44
    y1 = AttackedGeneralLoop(CLAIMS[name][0], [0, 1, 2, 3], *GEOM44, "hann", SR).embed(audio, wm)[0].numpy()
    claim(name, lambda z: ber(plain, bits, z), y0, y1)


# ---- 4. parse and carve on the CPU ------------------------------------------------------------------------------------------------------
def general_chain_check():
    """tests/host_sim/general_chain_check.cpp, built without HIP where it is missing or older than its sources.  Returns
    run(text) -> [(return code, bytes)], one pair per chain of the program's input."""
    exe = os.path.join(ROOT, "tests", "host_sim", "general_chain_check")
    src = os.path.join(ROOT, "tests", "host_sim", "general_chain_check.cpp")
    hdrs = [os.path.join(ROOT, "aware_amd", "csrc", h) for h in ("loop_any_chain.hpp", "loop_chain.hpp", "loop_limits.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [src] + hdrs):
        cxx = ["g++", "-O2", "-std=c++17"] if shutil.which("g++") else ["hipcc", "-O2", "-std=c++17", "-x", "hip", "--offload-host-only"]
        subprocess.run(cxx + ["-o", exe, src], check=True)

    def run(text):
        out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.split()
        return list(zip(map(int, out[0::2]), map(int, out[1::2])))

    return run


def _entries(entries):
    return f"chain {len(entries)}\n" + "".join(f"{k} {pr!r} " + " ".join(repr(float(x)) for x in (list(p) + [0.0] * 4)[:4]) + "\n"
                                               for k, pr, p in entries)


def _dims(d):
    return f"dims {d['B']} {d['NS']} {d['NF']} {d['pstride']} " + " ".join(str(n) for n in d["out_len"]) + "\n"


def expected_bytes(d):
    """The carve of loop_any_chain.hpp restated: z [NS] f32, pmaxZ [B][np] u64, psq [4][B][np] f64, pdotA, pdotX [B][np] f64,
    seeds [B] u32, each at the next multiple of 256 bytes; np = pieces of 3072 samples of the longest clip."""
    np_ = max(1, -(-max(d["out_len"]) // 3072))
    off = 0
    for count, size in ((d["NS"], 4), (d["B"] * np_, 8), (d["B"] * np_ * 4, 8), (d["B"] * np_, 8), (d["B"] * np_, 8), (d["B"], 4)):
        off = ((off + 255) & ~255) + count * size
    return off


def test_c_parser_and_carver_on_the_cpu():
    """csrc/loop_any_chain.hpp through tests/host_sim/general_chain_check (built without HIP): the setter's return codes, and the
    workspace size for the dims of tests/golden/loop_kinds_table.json."""
    run = general_chain_check()
    with open(os.path.join(ROOT, "tests", "golden", "loop_kinds_table.json")) as f:
        golden = json.load(f)
    dims = [v for v in _find_dims(golden)]
    assert dims, "the fixture holds batch dimensions"
    # ... and a batch at hop 75: odd offsets and lengths, a clip of exactly one piece, one of a piece and a hop, a short one
    odd = [3075, 3072 + 75 - 72, 150, 9225]
    dims.append({"B": 4, "NS": sum(odd), "NF": sum(n // 75 + 1 for n in odd), "pstride": 3, "out_len": odd})
    NO, EV = (0, 1.0, [10.0]), (8, 0.75, [800.0, 8000.0, 0.25])
    for d in dims:
        kmax = min(d["out_len"])
        SU = (1, 0.75, [float(kmax // 2)])
        ok = [[NO], [SU], [EV], [SU, NO], [NO, SU], [EV, SU, NO, EV]]
        got = run(_dims(d) + "".join(_entries(e) for e in ok))
        assert got == [(0, expected_bytes(d))] * len(ok), (d, got)
        other = {k: LA.device_entries_ex(LA.parse_chain([a]), 16000)[0] for k, a in ONE_OF_EACH.items()}
        bad = [([], -1), ([NO] * 5, -1), ([(0, 1.5, [10.0])], -1), ([(0, 1.0, [float("nan")])], -1), ([(13, 1.0, [0.0])], -1),
               ([(-1, 1.0, [0.0])], -1), ([(1, 1.0, [0.5])], -1), ([(8, 1.0, [32.0, 8000.0, 0.0])], -1), ([(8, 1.0, [800.0, 8000.0, 1.0])], -1),
               ([(3, 1.0, [5.0, 1.0])], -1),                          # a malformed entry of a kind that is not served: bad first
               ([(1, 1.0, [float(kmax)])], -2), ([NO, (1, 1.0, [float(kmax + 7)])], -2), ([(1, 1.0, [float(kmax - 1)])], 0)]
        bad += [([e], -2) for e in other.values()] + [([NO, e], -2) for e in other.values()]
        got = run(_dims(d) + "".join(_entries(e) for e, _ in bad))
        for (e, want), (rc, nbytes) in zip(bad, got):
            assert rc == want, (d, e, rc, want)
            assert nbytes == (0 if rc == -1 else expected_bytes(d)), (d, e, rc, nbytes)
        # the workspace check of the setter: the size fits, one byte less does not (AWARE_E_WORKSPACE)
        nb = expected_bytes(d)
        pieces = max(1, -(-max(d["out_len"]) // 3072))
        assert run(_dims(d) + f"carve {nb}\ncarve {nb - 1}\n") == [(1, pieces), (0, pieces)]


def _find_dims(node):
    """every {"B", "NS", "NF", "pstride", "out_len"} object of the fixture"""
    if isinstance(node, dict):
        if {"B", "NS", "NF", "pstride", "out_len"} <= set(node):
            yield node
        for v in node.values():
            yield from _find_dims(v)
    elif isinstance(node, list):
        for v in node:
            yield from _find_dims(v)
