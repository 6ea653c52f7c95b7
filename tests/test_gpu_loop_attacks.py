"""Attack-aware embedding (EXTENSION) on the device: the chain kernels of csrc/loop_attack_kernels.hip inside the embed loop
against the torch restatement aware_amd/embedding/loop_attacks.py::apply_chain composed with the oracle's loop body.

Run on the MI355X box:  python -m pytest tests/test_gpu_loop_attacks.py -m gpu -q -s"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import make_clip
from loop_support import LA, NOISE10, O, SUP, attacked, check_first_gradient, graph_replay_bits, norm2, rt, sampled, session
from loop_support import synthesis, value_claim_setup

pytestmark = pytest.mark.gpu

NOISE5 = {"kind": "gaussian_noise", "snr_db": 5.0}
CHAINS = {"noise10": [NOISE10], "noise5": [NOISE5], "suppression": [SUP], "suppression_noise": [SUP, NOISE10],
          "noise_suppression": [NOISE5, SUP]}


# ---- 4. forward ---------------------------------------------------------------------------------------------------------------
def check_forward(LA, sess, batch, chain, seeds, step, tag, sample=None):
    torch.cuda.synchronize()
    worst = 0.0
    for b, y, z in sampled(sess, batch, sample):
        ref = LA.apply_chain(norm2(y.double())[None], chain, [seeds[b]], step)[0]
        np.testing.assert_array_equal((z == 0).numpy(), (ref == 0).numpy())       # suppressed samples: exact zeros, same places
        worst = max(worst, float((z.double() - ref).abs().max()))
    print(f"{tag}, step {step}: max |z - restatement| = {worst:.2e}")
    assert worst < 1e-6, (tag, step, worst)


@pytest.mark.parametrize("name", list(CHAINS))
@pytest.mark.parametrize("lengths", [[16000] * 8, [16000, 40000, 64000]])
def test_forward_matches_the_restatement(rt, O, LA, name, lengths):
    """Buffer 12 against apply_chain(N(N(buffer 9))) at steps 0, 2 (after three steps) and 16 (after seventeen): zeros exactly
    where the restatement has them, every other sample within 1e-6 of a unit-peak signal."""
    chain = CHAINS[name]
    seeds = [11 + 3 * i for i in range(len(lengths))]
    sess, batch, _, _ = session(rt, O, lengths, list(range(20, 20 + len(lengths))), chain, seeds, num_iterations=20)
    sess.gradient()
    check_forward(LA, sess, batch, chain, seeds, 0, name)
    sess.iterate(3)
    assert int(sess.step.cpu()[0]) == 3
    check_forward(LA, sess, batch, chain, seeds, 2, name)
    sess.iterate(14)
    check_forward(LA, sess, batch, chain, seeds, 16, name)
    sess.gradient()                                           # evaluates the current step, 17, without advancing it
    check_forward(LA, sess, batch, chain, seeds, 17, name)
    assert int(sess.step.cpu()[0]) == 17


@pytest.mark.parametrize("lengths", [[16000] * 8, [16000, 40000, 64000]])
def test_step_0_matches_the_device_attacks(rt, O, LA, lengths):
    """At step 0 and chain index 0 the loop's noise is rt.gaussian_noise of the same seeds and its suppression rt.segment_cut
    at the drawn starts.  Tolerance of the noise: the 2e-7 of test_gaussian_noise_extension, whose clips peak at 0.41,
    scaled to the unit peak of the loop's signal."""
    a, _ = make_clip(4, 16000)
    b, _ = make_clip(5, 20000)
    atol = 2e-7 / max(np.abs(a).max(), np.abs(b).max())
    seeds = [3 + i for i in range(len(lengths))]
    for snr in (10.0, 5.0):
        sess, batch, _, _ = session(rt, O, lengths, list(range(30, 30 + len(lengths))), [{"kind": "gaussian_noise", "snr_db": snr}], seeds)
        sess.gradient()
        torch.cuda.synchronize()
        xs = [norm2(y).float() for y in synthesis(sess, batch)]
        ref = rt.gaussian_noise(rt.Ragged.from_list([x.numpy() for x in xs]), snr, seeds).to_list()
        err = max(float(np.abs(z.numpy().astype(np.float64) - r.astype(np.float64)).max()) for z, r in zip(attacked(sess, batch), ref))
        print(f"noise {snr} dB against rt.gaussian_noise: max error {err:.2e} (bound {atol:.2e})")
        assert err < atol
    sess, batch, _, _ = session(rt, O, lengths, list(range(30, 30 + len(lengths))), [SUP], seeds)
    sess.gradient()
    torch.cuda.synchronize()
    xs = [norm2(y).float() for y in synthesis(sess, batch)]
    starts = [LA.suppression_start(LA.entry_draw(s, 0, 0)[1], n, 4800) for s, n in zip(seeds, batch.out_lengths)]
    ref = rt.segment_cut(rt.Ragged.from_list([x.numpy() for x in xs]), starts, [4800] * batch.B, zero_fill=True).to_list()
    for z, r, st in zip(attacked(sess, batch), ref, starts):
        assert np.all(z.numpy()[st:st + 4800] == 0) and np.all(r[st:st + 4800] == 0)
        np.testing.assert_array_equal((z == 0).numpy(), r == 0)
        np.testing.assert_allclose(z.numpy(), r, atol=3e-7)           # x itself: five f32 roundings (3 device, 2 host) at unit peak


# ---- 5. first gradient ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["noise10", "suppression", "suppression_noise", "noise_suppression"])
@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
def test_first_gradient(rt, O, LA, name, dsp_path):
    """aware_embed_gradient with a chain against torch autograd over the restatement composed with the oracle's loop body:
    2e-5 relative L2 per clip (2e-2 for a clip with a LeakyReLU argument within 2e-6 of its kink), loss and prediction 1e-5."""
    check_first_gradient(rt, O, LA, CHAINS[name], [16000, 16000 + 256 * 9], dsp_path=dsp_path)


@pytest.mark.parametrize("kw", [dict(mel="dense"), dict(conv_pipe="f32"), dict(conv_pipe="f16x2", mel="taps"),
                                dict(dsp_path="staged", mel="dense", conv_pipe="f32")])
def test_first_gradient_variants(rt, O, LA, kw):
    check_first_gradient(rt, O, LA, CHAINS["suppression_noise"], [16000, 20000], **kw)


@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
def test_first_gradient_ragged(rt, O, LA, dsp_path):
    check_first_gradient(rt, O, LA, CHAINS["noise_suppression"], [16000, 40000, 64000, 8000], dsp_path=dsp_path)


@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
def test_first_gradient_wide_band(rt, O, LA, dsp_path):
    check_first_gradient(rt, O, LA, CHAINS["suppression_noise"], [16000, 24000], band=(0, 512), dsp_path=dsp_path)


# ---- 6. graph replay ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", [[16000] * 4, [16000, 40000]])
def test_graph_replay_is_bit_identical_and_redraws(rt, O, lengths):
    chain = [{"kind": "sample_suppression", "seconds": 0.3, "prob": 0.75}, NOISE10]
    out, _ = graph_replay_bits(rt, O, chain, lengths)
    zs = out[4]
    for i in range(7):
        assert float((zs[i + 1] - zs[i]).abs().max()) > 1e-2        # the draw is keyed by the device step counter


# ---- 7. no chain, cleared chain, prob 0 -----------------------------------------------------------------------------------------
def test_no_chain_is_the_plain_loop(rt, O):
    lengths = [16000, 24000]
    res = []
    for mode in ("never", "cleared", "empty"):
        sess, batch, _, _ = session(rt, O, lengths, [60, 61], None, num_iterations=20)
        if mode == "cleared":
            sess.set_loop_attacks([NOISE10, SUP], [1, 2])
            sess.set_loop_attacks([], [])
        elif mode == "empty":
            sess.set_loop_attacks(None, [])
        assert sess.attacked is None
        sess.iterate(20)
        torch.cuda.synchronize()
        res.append((sess.coef.cpu(), sess.best_coef.cpu(), sess.loss.cpu()))
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.equal(a, b)


def test_prob_0_runs_the_path_and_changes_nothing(rt, O):
    lengths = [16000, 24000]
    plain, _, _, _ = session(rt, O, lengths, [62, 63], None, num_iterations=20)
    chain = [{"kind": "gaussian_noise", "snr_db": 5.0, "prob": 0.0}, {"kind": "sample_suppression", "seconds": 0.5, "prob": 0.0}]
    att, batch, _, _ = session(rt, O, lengths, [62, 63], chain, num_iterations=20)
    plain.iterate(1)
    att.iterate(1)
    torch.cuda.synchronize()
    d = float((plain.loss - att.loss).abs().max())
    print("first-step loss, prob 0 against the plain loop:", d)
    assert d < 1e-6
    zs, ys = attacked(att, batch), synthesis(att, batch)
    for z, y in zip(zs, ys):
        assert float((z.double() - norm2(y.double())).abs().max()) < 2e-7
    gp, ga = plain.gradient(), att.gradient()
    assert float((gp - ga).norm() / gp.norm()) < 2e-5


# ---- 8. error codes -------------------------------------------------------------------------------------------------------------
def test_entry_point_error_codes(rt, O):
    from aware_amd._lib import LoopAttack
    sess, batch, _, _ = session(rt, O, [16000, 8000], [64, 65], None, num_iterations=4, use_graph=False)
    lib = sess.lib
    nbytes = lib.aware_embed_loop_attack_workspace_bytes(batch.h, 1)
    assert nbytes >= 4 * batch.total_out
    assert lib.aware_embed_loop_attack_workspace_bytes(batch.h, 0) == 0 and lib.aware_embed_loop_attack_workspace_bytes(batch.h, 5) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    seeds = (C.c_uint32 * 2)(1, 2)

    def call(entries, n=None, wsb=nbytes, sd=seeds):
        arr = (LoopAttack * max(1, len(entries)))(*[LoopAttack(*e) for e in entries])
        return lib.aware_embed_set_loop_attacks(sess.h, arr, len(entries) if n is None else n, sd, C.c_void_p(ws.data_ptr()), wsb, None)

    assert call([(2, 10.0, 1.0)]) == -1                       # unknown kind
    assert call([(0, 10.0, 1.0)], n=5) == -1 and call([(0, 10.0, 1.0)], n=-1) == -1
    assert call([(0, 10.0, 1.5)]) == -1 and call([(1, 100.0, -0.5)]) == -1 and call([(0, 10.0, float("nan"))]) == -1
    assert call([(0, float("inf"), 1.0)]) == -1 and call([(0, float("nan"), 1.0)]) == -1
    assert call([(1, 0.0, 1.0)]) == -1                        # k < 1
    assert call([(1, 7936.0, 1.0)]) == -2                     # k >= Ny of the 8000-sample clip (7936 output samples)
    assert call([(1, 7935.0, 1.0)]) == 0
    assert call([(0, 10.0, 1.0)], wsb=nbytes - 1) == -4
    assert call([(0, 10.0, 1.0)], sd=None) == -1
    assert call([(0, 10.0, 1.0), (1, 4800.0, 0.75)]) == 0
    assert lib.aware_embed_buffer(sess.h, 12)
    assert call([], n=0) == 0 and not lib.aware_embed_buffer(sess.h, 12)
    with pytest.raises(ValueError, match="clip 1"):
        sess.set_loop_attacks([{"kind": "sample_suppression", "seconds": 0.5}], [1, 2])
    sess.iterate(1)
    assert call([(0, 10.0, 1.0)]) == -1                       # after the first iterate
    assert call([], n=0) == -1
    with pytest.raises(ValueError):
        sess.set_loop_attacks([NOISE10], [1, 2])


# ---- 9. the value claim on the device ---------------------------------------------------------------------------------------------
def test_value_claim_on_the_device(rt, O, tmp_path):
    """Four 1 s clips, seeds 0..3, 400 steps through AWAREEmbedder(loop_attacks=...): clean BER 0 %; BER under noise at 5 dB SNR
    (8 seeds per clip) of the noise-aware embedding at most half the plain one's, which is at least 10 %; the same for
    0.5 s zeroed at six starts with sample_suppression(0.5 s, prob 0.75) in the loop."""
    from aware_amd import attacks as A
    clips, bits, embed, ber = value_claim_setup(O, tmp_path)

    def noise5(det, ys):
        x = rt.Ragged.from_list(ys)
        return float(np.mean([ber(det, A.GaussianNoise(5.0).apply_batch(x, 16000, seeds=[1000 * sd + b for b in range(4)]))
                              for sd in range(8)]))

    def half_zeroed(det, ys):
        x = rt.Ragged.from_list(ys)
        return float(np.mean([ber(det, A.SampleSupression(0.5).apply_batch(x, 16000, starts=[st] * 4))
                              for st in (0, 1500, 3000, 4500, 6000, 7800)]))

    y0, det = embed(None)
    y1, _ = embed([{"kind": "gaussian_noise", "snr_db": 10.0}])
    y2, _ = embed([{"kind": "sample_suppression", "seconds": 0.5, "prob": 0.75}])
    c0, c1, c2 = ber(det, y0), ber(det, y1), ber(det, y2)
    n0, n1 = noise5(det, y0), noise5(det, y1)
    s0, s2 = half_zeroed(det, y0), half_zeroed(det, y2)
    print(f"clean BER: plain {c0:.2f} %, noise-aware {c1:.2f} %, suppression-aware {c2:.2f} %")
    print(f"noise at 5 dB: plain {n0:.2f} %, noise-aware {n1:.2f} %;  0.5 s zeroed: plain {s0:.2f} %, suppression-aware {s2:.2f} %")
    assert c0 == 0.0 and c1 == 0.0 and c2 == 0.0
    assert n0 >= 10.0 and n1 <= 0.5 * n0
    assert s0 >= 10.0 and s2 <= 0.5 * s0
