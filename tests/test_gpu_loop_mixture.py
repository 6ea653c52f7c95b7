"""Attack mixtures (EXTENSION) on the device: the draw, a mixture against its chains clip by clip, later
steps against the torch restatement, one chain of weight 1, graph replay, a single-chain handle against the record of the
loop before mixtures, the workspace and the error codes, the service, and the value claim."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, make_clip
from loop_support import CHAIN_BOUND, LA, NO, O, RV, SU, attacked, mixture_session as session, norm2, rows, rt, span, synthesis, weights
from test_loop_mixture_host import CENTS, CROPS, FAMILIES, HALF_OF_PLAIN, MIX, MIX2, RATES

pytestmark = pytest.mark.gpu

assert CHAIN_BOUND == 1.13e-6                              # the project's bound for the loop's attacked signal
UNIFORM = [16000] * 10
RAGGED = [16000, 8000, 24000, 23456, 12001, 16000, 9000, 31999, 16384, 20000]
MIXTURES = {"four_families": MIX, "tempo_pitch": MIX2}
KINDS01 = [{"kind": "sample_suppression", "seconds": 0.3, "prob": 0.75}, {"kind": "gaussian_noise", "snr_db": 10.0}]
REVERB = [{"kind": "reverberation", "rt60": [0.1, 0.5], "drr_db": -3.0, "prob": 0.75}, {"kind": "gaussian_noise", "snr_db": 20.0}]
PITCH = [{"kind": "pitch_shift", "cents": 100.0, "prob": 0.75}]
HALF_OF_PLAIN_DEVICE = tuple(k for k in HALF_OF_PLAIN if k != "rooms of rt60 0.3 s")


def covering_seeds(LA, mixture, n=10):
    """The first run of n seeds >= 100 in which every option of the mixture, -1 included if it has a clean share, occurs at step 0."""
    w = weights(mixture)
    want = set(range(len(w))) | ({-1} if sum(w) < 1.0 - 1e-6 else set())
    s0 = 100
    while set(LA.mixture_choices(range(s0, s0 + n), 0, w).tolist()) != want:
        s0 += 1
    seeds = list(range(s0, s0 + n))
    assert set(LA.mixture_choices(seeds, 0, w).tolist()) == want       # the coverage the tests below rely on
    return seeds


# ---- 1. the draw ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [[0.2] * 4, [0.1, 0.0, 0.6], [0.4, 0.3, 0.3], [0.5, 0.5], [1.0], [0.25], [0.05] * 8])
def test_draw_is_the_host_twin(rt, LA, w):
    """aware_loop_mixture_draw against mixture_choice, exactly, for 64 seeds at steps 0, 1 and 399: with a zero weight, with a sum
    of 1 (no clean share), with a single chain, with eight chains; seeds up to 2^32 - 1."""
    seeds = list(range(61)) + [2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1]
    for step in (0, 1, 399):
        got = rt.loop_mixture_draw(seeds, step, w).cpu().numpy()
        np.testing.assert_array_equal(got, LA.mixture_choices(seeds, step, w))
    with pytest.raises(ValueError):
        rt.loop_mixture_draw(seeds, 0, [0.6, 0.5])


# ---- 2. a mixture is its chains ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
@pytest.mark.parametrize("lengths", [UNIFORM, RAGGED], ids=["uniform", "ragged"])
@pytest.mark.parametrize("name", list(MIXTURES))
def test_a_mixture_is_its_chains(rt, O, LA, name, lengths, dsp_path):
    """gradient() at step 0 under the mixture against, per clip, a session that holds only the chain the clip drew (the same
    clips, the same attack seeds): the clip's samples of buffers 12 and 9, its loss, its prediction and its rows of the
    coefficient gradient, bit for bit.  A clip that drew no chain: against the session without loop attacks, by the rule of
    test_prob_0_is_the_plain_loop (z within 2e-7 of N(N(y)), everything else bit for bit)."""
    mixture = LA.parse_mixture(MIXTURES[name])
    seeds = covering_seeds(LA, mixture)
    choice = LA.mixture_choices(seeds, 0, weights(mixture))
    kw = dict(num_iterations=4, dsp_path=dsp_path)
    mix, batch = session(rt, O, lengths, seeds, mixture=mixture, **kw)
    g = mix.gradient()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(mix.choices.cpu().numpy(), choice)
    z, y, loss, pred = mix.attacked.clone(), mix._view(9, (batch.total_out,)).clone(), mix.loss.clone(), mix.pred.clone()
    for c in sorted(set(choice.tolist())):
        one, _ = session(rt, O, lengths, seeds, chain=mixture[c]["chain"] if c >= 0 else None, **kw)
        g1 = one.gradient()
        torch.cuda.synchronize()
        y1 = one._view(9, (batch.total_out,))
        for b in np.flatnonzero(choice == c):
            tag = (name, dsp_path, int(b), c)
            assert torch.equal(y[span(batch, b)], y1[span(batch, b)]), tag
            if c >= 0:
                assert torch.equal(z[span(batch, b)], one.attacked[span(batch, b)]), tag
            else:
                assert float((z[span(batch, b)].double() - norm2(y[span(batch, b)].double())).abs().max()) < 2e-7, tag
            assert torch.equal(loss[b], one.loss[b]) and torch.equal(pred[b], one.pred[b]), tag
            assert torch.equal(g[rows(batch, b)], g1[rows(batch, b)]), (tag, float((g[rows(batch, b)] - g1[rows(batch, b)]).abs().max()))
            assert float(g[rows(batch, b)].abs().max()) > 0.0


# ---- 3. later steps ---------------------------------------------------------------------------------------------------------------
def check_forward(LA, sess, batch, mixture, seeds, step, tag):
    """Buffer 12 against apply_mixture on N(N(buffer 9)) in float64, per clip by the bound of its chain's own GPU test: the
    project's CHAIN_BOUND of the reference's peak; a clip through the phase vocoder by test_gpu_loop_pv's rule, four times the
    float32 restatement's distance from the float64 one where that is more; a clip that drew no chain within 2e-7 of N(N(y))."""
    torch.cuda.synchronize()
    choice = LA.mixture_choices(seeds, step, weights(mixture))
    np.testing.assert_array_equal(sess.choices.cpu().numpy(), choice)
    worst = 0.0
    for b, (y, z) in enumerate(zip(synthesis(sess, batch), attacked(sess, batch))):
        x = norm2(y.double())
        ref = LA.apply_mixture(x[None], mixture, [seeds[b]], step)[0]
        err = float((z.double() - ref).abs().max()) / float(ref.abs().max())
        bound = CHAIN_BOUND
        if choice[b] < 0:
            bound = 2e-7 / float(ref.abs().max())
        elif any(a["kind"] == "phase_vocoder" for a in mixture[choice[b]]["chain"]):
            r32 = LA.apply_mixture(x.float()[None], mixture, [seeds[b]], step)[0]
            bound = max(4 * float((r32.double() - ref).abs().max()) / float(ref.abs().max()), CHAIN_BOUND)
        worst = max(worst, err)
        assert err <= bound, (tag, step, b, int(choice[b]), err, bound)
    print(f"{tag}, step {step}: choices {choice.tolist()}, max |z - restatement| / peak = {worst:.2e}")


@pytest.mark.parametrize("lengths", [UNIFORM, RAGGED], ids=["uniform", "ragged"])
@pytest.mark.parametrize("name", list(MIXTURES))
def test_later_steps_match_the_restatement(rt, O, LA, name, lengths):
    mixture = LA.parse_mixture(MIXTURES[name])
    seeds = covering_seeds(LA, mixture)
    sess, batch = session(rt, O, lengths, seeds, mixture=mixture, num_iterations=20)
    sess.iterate(3)
    check_forward(LA, sess, batch, mixture, seeds, 2, name)
    sess.iterate(14)
    check_forward(LA, sess, batch, mixture, seeds, 16, name)


# ---- 4. one chain of weight 1 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [KINDS01, REVERB], ids=["kinds01", "reverberation"])
def test_one_chain_of_weight_1_is_the_chain(rt, O, LA, chain):
    """20 iterations of [{weight 1, chain}] against set_loop_attacks with the same chain: coefficients, best coefficients,
    losses and the finished waveform, bit for bit."""
    seeds = list(range(30, 40))
    out = []
    for as_mixture in (True, False):
        sess, batch = session(rt, O, RAGGED, seeds, num_iterations=20,
                              **({"mixture": [{"weight": 1.0, "chain": chain}]} if as_mixture else {"chain": chain}))
        sess.iterate(20)
        torch.cuda.synchronize()
        if as_mixture:
            assert sess.choices.cpu().tolist() == [0] * 10
        out.append((sess.coef.cpu(), sess.best_coef.cpu(), sess.loss.cpu(), sess.best_loss.cpu(), sess.attacked.cpu(), sess.finish(None).cpu()))
    for a, b in zip(*out):
        assert torch.equal(a, b)


# ---- 5. graph replay --------------------------------------------------------------------------------------------------------------
def test_graph_replay_is_bit_identical_and_redraws(rt, O, LA):
    mixture = LA.parse_mixture(MIX)
    seeds = covering_seeds(LA, mixture)
    w = weights(mixture)
    per_step = [LA.mixture_choices(seeds, s, w).tolist() for s in (15, 16, 17)]
    assert any(len({c[b] for c in per_step}) == 3 for b in range(10))  # a clip whose three choices differ: the second recorded body redraws
    out = []
    for use_graph in (True, False):
        sess, batch = session(rt, O, RAGGED, seeds, mixture=mixture, num_iterations=40, use_graph=use_graph)
        zs, losses, choices = [], [], []
        sess.iterate(15)
        for _ in range(3):
            sess.iterate(1)
            zs.append(sess.attacked.clone()); losses.append(sess.loss.clone()); choices.append(sess.choices.clone())
        sess.iterate(22)
        torch.cuda.synchronize()
        assert int(sess.step.cpu()[0]) == 40
        assert [c.cpu().tolist() for c in choices] == per_step
        out.append((sess.coef.cpu(), sess.best_coef.cpu(), sess.best_loss.cpu(), torch.stack(losses).cpu(), torch.stack(zs).cpu(),
                    sess.finish(None).cpu()))
    for a, b in zip(*out):
        assert torch.equal(a, b)


# ---- 6. a single-chain handle is untouched ----------------------------------------------------------------------------------------
def test_single_chain_handles_keep_their_bits(rt, O):
    """tools/loop_attack_bench.py --dump on this tree against tests/golden/loop_single_chain_sha256.json, recorded with the
    same tool on the commit before mixtures: 20 iterations of a kind-0/1 chain and of a pitch-shift chain on ten 1 s clips,
    sha256 of the coefficients, the best coefficients, the losses and the finished waveform."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("loop_attack_bench", os.path.join(ROOT, "tools", "loop_attack_bench.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    from aware_amd.utils.models import load
    emb, _ = load()
    emb.verbose = False
    got = tool.dump(emb, None)
    with open(os.path.join(ROOT, "tests", "golden", "loop_single_chain_sha256.json")) as f:
        want = json.load(f)
    assert got == want


def test_every_chain_keeps_its_bits(rt, O, LA):
    """tests/golden/loop_chains_sha256.json, recorded with the same tool on the commit before the chains' host logic moved into
    csrc/loop_chain.hpp: every chain of VARIANTS and both MIXTURES, 8 iterations on three ragged clips (24 draws per entry, so
    every entry of prob 0.75 fires and idles), sha256 of the coefficients, the best coefficients, the losses and the finished
    waveform; and the two workspace byte counts of the C ABI for the same chains on that batch and on [16000, 8000]."""
    import importlib.util
    from aware_amd._lib import LoopAttackEx
    spec = importlib.util.spec_from_file_location("loop_attack_bench", os.path.join(ROOT, "tools", "loop_attack_bench.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "tests", "golden", "loop_chains_sha256.json")) as f:
        want = json.load(f)
    names = [k for k in tool.VARIANTS if k != "none"] + list(tool.MIXTURES)
    assert want["names"] == names and len(names) == 15 and want["lengths"] == [16000, 12000, 9000] and want["iters"] == 8
    emb, _ = load()
    emb.verbose = False
    got = tool.dump(emb, None, names=names, lengths=want["lengths"], iters=want["iters"])
    for name in names:
        assert got[name] == want["sha256"][name], name
    for ws in want["workspace"]:
        batch = rt.Batch(ws["lengths"])
        assert (batch.B, batch.total_out, batch.total_frames, batch.out_lengths) == \
            (ws["dims"]["B"], ws["dims"]["NS"], ws["dims"]["NF"], ws["dims"]["out_len"])
        assert len(ws["bytes"]) == (15 if ws["lengths"] == want["lengths"] else 14)
        for name, nbytes in ws["bytes"].items():
            if name in tool.VARIANTS:
                ent = LA.device_entries_ex(LA.parse_chain(tool.VARIANTS[name]), 16000)
                arr = (LoopAttackEx * len(ent))(*[LoopAttackEx(k, pr, (C.c_float * 4)(*p)) for k, pr, p in ent])
                assert batch.lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, arr, len(ent)) == nbytes, (ws["lengths"], name)
            else:
                arr, keep = chains_struct(rt, LA, tool.MIXTURES[name])
                assert batch.lib.aware_embed_loop_mixture_workspace_bytes(batch.h, arr, len(arr)) == nbytes, (ws["lengths"], name)


# ---- 7. workspace and errors ------------------------------------------------------------------------------------------------------
def chains_struct(rt, LA, mixture, sample_rate=16000):
    return rt.mixture_struct([(m["weight"], LA.device_entries_ex(LA.parse_chain(m["chain"]), sample_rate)) for m in mixture])


def test_workspace_and_error_codes(rt, O, LA):
    from aware_amd._lib import LoopAttackEx, LoopChain
    lengths = [16000, 8000]
    sess, batch = session(rt, O, lengths, num_iterations=4, use_graph=False)
    lib = sess.lib
    # one chain: the chain's own workspace, rounded up to 256, then int [B] choices
    for chain in (KINDS01, REVERB, MIX[2]["chain"], MIX2[0]["chain"], PITCH):
        arr, keep = chains_struct(rt, LA, [{"weight": 1.0, "chain": chain}])
        ent = keep[0]
        ex = lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ent, len(ent))
        assert lib.aware_embed_loop_mixture_workspace_bytes(batch.h, arr, 1) == ((ex + 255) & ~255) + 4 * batch.B
    arr, keep = chains_struct(rt, LA, MIX)
    nbytes = lib.aware_embed_loop_mixture_workspace_bytes(batch.h, arr, 4)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    seeds = (C.c_uint32 * 2)(1, 2)

    def call(arr, n, wsb=nbytes, sd=seeds, w=ws):
        return lib.aware_embed_set_loop_mixture(sess.h, arr, n, sd, C.c_void_p(w.data_ptr()) if w is not None else None, wsb, None)

    def mix_of(entries_and_weights):
        keep = [(LoopAttackEx * max(1, len(e)))(*[LoopAttackEx(k, pr, (C.c_float * 4)(*(list(p) + [0.0] * (4 - len(p))))) for k, pr, p in e])
                for e, _ in entries_and_weights]
        return (LoopChain * len(keep))(*[LoopChain(C.cast(a, C.POINTER(LoopAttackEx)), len(e), w)
                                         for a, (e, w) in zip(keep, entries_and_weights)]), keep

    DS, SP = (7, 1.0, [1.0, 512.0, 1.0]), (3, 1.0, [-3678.0, 3896.0])
    assert call(arr, 4) == 0 and lib.aware_embed_buffer(sess.h, 14) and lib.aware_embed_buffer(sess.h, 12) and lib.aware_embed_buffer(sess.h, 13)
    assert call(arr, 4, wsb=nbytes - 1) == -4
    assert call(arr, 9) == -1 and call(arr, -1) == -1
    assert call(None, 1) == -1 and call(arr, 4, sd=None) == -1 and call(arr, 4, w=None) == -1
    for bad, rc in (([([], 0.5)], -1),                                           # an empty chain
                    ([([NO], -0.1)], -1), ([([NO], float("nan"))], -1), ([([NO], float("inf"))], -1),
                    ([([NO], 0.6), ([SU], 0.5)], -1),                            # a sum above 1
                    ([([NO], 0.5), ([(9, 1.0, [0.0])], 0.5)], -1),               # what the _ex setter refuses, per chain
                    ([([NO], 0.5), ([DS, SP], 0.5)], -1),                        # two kinds that split one chain
                    ([([NO] * 5, 0.5)], -1),
                    ([([RV], 0.5), ([RV, NO], 0.5)], -1),                        # a second reverberation chain
                    ([([NO], 0.5), ([(1, 1.0, [7936.0])], 0.5)], -2)):           # k >= Ny of the 8000-sample clip
        a, k = mix_of(bad)
        assert call(a, len(bad)) == rc, bad
        assert lib.aware_embed_loop_mixture_workspace_bytes(batch.h, a, len(bad)) == 0 or rc == -2
    a, k = mix_of([([NO], 0.5), ([SU], 0.5 + 5e-7)])
    assert call(a, 2) == 0                                                       # a sum within 1 + 1e-6
    assert not lib.aware_embed_buffer(sess.h, 13)                                # no reverberation chain
    # a mixture and a plain chain replace each other; n_chains = 0 restores the plain loop
    sess.set_loop_attacks(KINDS01, [1, 2])
    assert not lib.aware_embed_buffer(sess.h, 14) and lib.aware_embed_buffer(sess.h, 12)
    sess.set_loop_mixture(MIX, [1, 2])
    assert lib.aware_embed_buffer(sess.h, 14)
    sess.set_loop_mixture([], [])
    assert sess.choices is None and sess.attacked is None
    plain, _ = session(rt, O, lengths, num_iterations=4, use_graph=False)
    sess.iterate(3)
    plain.iterate(3)
    torch.cuda.synchronize()
    assert torch.equal(sess.coef, plain.coef) and torch.equal(sess.loss, plain.loss)
    assert call(arr, 4) == -1 and call(arr, 0) == -1                             # after the first iterate
    with pytest.raises(ValueError):
        sess.set_loop_mixture(MIX, [1, 2])
    with pytest.raises(ValueError, match=r"loop_attack_mixture\[0\].*clip 1"):
        s2, _ = session(rt, O, [16000, 4000], num_iterations=4)
        s2.set_loop_mixture(MIX, [1, 2])


# ---- 8. the service ---------------------------------------------------------------------------------------------------------------
def test_service_with_a_mixture_on_the_card(rt, O, tmp_path):
    from aware_amd.service import detect_watermark, embed_watermark
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        card = yaml.safe_load(f)
    card["loop_attack_mixture"] = MIX
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert len(emb.loop_attack_mixture) == 4
    left, bits = make_clip(300, 16000)
    right, _ = make_clip(301, 16000)
    out = embed_watermark(np.column_stack([left, right]), 16000, bits, emb)        # stereo: every channel through the mixture
    assert out.ndim == 2 and out.shape[1] == 2
    for ch in range(2):
        np.testing.assert_array_equal(detect_watermark(np.ascontiguousarray(out[:, ch]), 16000, det), bits)


# ---- 9. the value claim on the device ---------------------------------------------------------------------------------------------
def test_value_claim_on_the_device(rt, O, tmp_path):
    """The host test's two embeddings through AWAREEmbedder (plain, and loop_attack_mixture = MIX), four 1 s clips, seeds 0..3,
    400 steps, evaluated at the host test's points with the device attacks where they exist (GaussianNoise, SampleSupression,
    TimeStretch, PitchShift; the fixed rooms through the host's responses and runtime.convolve; slicing for the dropped
    samples).  The same hard conditions: clean BER 0 % for both; on every family the mixture's mean at least 5 points below
    the plain watermark's; at most half of plain on the families that meet it on the device with 2.5 points to spare
    (HALF_OF_PLAIN_DEVICE).  Measured on the MI355X, plain / mixture: noise 23.75 / 2.34, zeroed 39.38 / 22.29, rooms 40.42 / 18.33,
    TimeStretch 35.00 / 5.00, PitchShift 51.25 / 42.19, dropped 23.00 / 2.00 %, clean 0 / 0.  Zeroed and PitchShift miss half of
    plain, as on the CPU; the rooms meet it with 1.9 points, less than the 2.5 that would make it an assertion here."""
    from aware_amd import attacks as A
    from aware_amd.utils.models import load
    from test_loop_reverb_host import room_response
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        card = yaml.safe_load(f)
    pairs = [make_clip(s, 16000) for s in range(4)]
    clips, bits = [p[0] for p in pairs], np.stack([p[1] for p in pairs])
    wm = np.stack([O.bits_to_bipolar(b) for b in bits]).astype(np.float32)

    def embed(mixture):
        c = dict(card)
        if mixture:
            c["loop_attack_mixture"] = mixture
        p = tmp_path / "card.yaml"
        p.write_text(yaml.safe_dump(c))
        emb, det = load(str(p))
        return [o.cpu().numpy() for o in emb.embed_batch(clips, 16000, wm)], det

    def ber(det, ragged):
        vals = det.detect_batch(ragged.to_list() if hasattr(ragged, "to_list") else ragged, 16000).cpu().numpy()
        return 100.0 * float((O.decode_bits(vals) != bits).mean())

    def table(det, ys):
        x = rt.Ragged.from_list(ys)
        rooms = []
        for s in range(3):
            h = room_response(s).astype(np.float32)
            hs = torch.from_numpy(np.stack([h] * 4)).cuda()
            rooms.append(ber(det, rt.convolve(x, hs, torch.full((4,), len(h), dtype=torch.int32, device="cuda"))))
        return {"noise at 5 dB": float(np.mean([ber(det, A.GaussianNoise(5.0).apply_batch(x, 16000, seeds=[1000 * sd + b for b in range(4)]))
                                                for sd in range(8)])),
                "half the clip zeroed": float(np.mean([ber(det, A.SampleSupression(0.5).apply_batch(x, 16000, starts=[st] * 4))
                                                       for st in (0, 1500, 3000, 4500, 6000, 7800)])),
                "rooms of rt60 0.3 s": float(np.mean(rooms)),
                "phase-vocoder TimeStretch": float(np.mean([ber(det, A.TimeStretch(rate=r).apply_batch(x, 16000)) for r in RATES])),
                "PitchShift": float(np.mean([ber(det, A.PitchShift(cents=c).apply_batch(x, 16000)) for c in CENTS])),
                "first samples dropped": float(np.mean([ber(det, [y[d:] for y in ys]) for d in CROPS]))}

    y0, det = embed(None)
    y1, _ = embed(MIX)
    c0, c1 = ber(det, y0), ber(det, y1)
    t0, t1 = table(det, y0), table(det, y1)
    print(f"clean BER plain {c0:.2f} % / mixture {c1:.2f} %")
    for k in FAMILIES:
        print(f"{k}: plain {t0[k]:.2f} % / mixture {t1[k]:.2f} %")
    assert c0 == 0.0 and c1 == 0.0
    for k in FAMILIES:
        assert t1[k] <= t0[k] - 5.0, (k, t0[k], t1[k])
    for k in HALF_OF_PLAIN_DEVICE:
        assert t1[k] <= 0.5 * t0[k], (k, t0[k], t1[k])
