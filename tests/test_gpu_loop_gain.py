"""Gain envelopes inside the embed loop and alone (EXTENSION, chain kind 8) on the device: csrc/loop_gain_kernels.hip against the
host model, the envelope inside the three stage kernels of csrc/loop_attack_kernels.hip against the torch restatement
aware_amd/embedding/loop_attacks.py::apply_chain composed with the oracle's loop body, graph replay, a mixture, the error codes,
and the value claim under fades, tremolo and ducking.

Run on the MI355X box:  python -m pytest tests/test_gpu_loop_gain.py -m gpu -q -s"""
import ctypes as C

import numpy as np
import pytest
import torch

from loop_support import LA, NOISE10, O, SUP, attacked, check_first_gradient, ex_entries, graph_replay_bits, mixture_session
from loop_support import norm2, rt, session, synthesis, value_claim_setup, weights
# the forward checks of the kinds an envelope's chains hold beside it, each from the module that owns it
from test_gpu_loop_attacks import check_forward as check_forward_01
from test_gpu_loop_reverb import check_forward as check_forward_reverb
from test_gpu_loop_mixture import check_forward as check_forward_mixture

pytestmark = pytest.mark.gpu

ENV = {"kind": "gain_envelope", "period": [0.05, 0.5], "prob": 0.75}
ENV_SHORT = {"kind": "gain_envelope", "period": 0.004, "floor": 0.25}          # 64 samples: the shortest period
REVERB = {"kind": "reverberation", "rt60": 0.3, "drr_db": -3.0}
CHAINS = {"envelope": [ENV], "envelope_noise": [ENV, NOISE10], "suppression_envelope": [SUP, ENV_SHORT],
          "envelope_reverb_envelope": [ENV, REVERB, ENV_SHORT], "envelope_prob_0": [dict(ENV, prob=0.0)]}
RAGGED, UNIFORM = [16000, 12000, 9000], [16000] * 32


# ---- 1. the operator alone ----------------------------------------------------------------------------------------------------
LENGTHS = [4099, 7937, 513, 16000]


@pytest.fixture(scope="module")
def clips():
    rng = np.random.default_rng(23)
    return [rng.standard_normal(n).astype(np.float32) for n in LENGTHS]


@pytest.mark.parametrize("floor", [0.0, 0.25])
@pytest.mark.parametrize("P", [64, 777, 20000])
def test_gain_envelope_against_the_host_model(rt, LA, clips, P, floor):
    """runtime.gain_envelope on ragged clips (one shorter than a workgroup's 4096 samples, one three samples longer, offsets that
    are no multiple of four) at steps 0 and 3, entries 0 and 2, against x g in float64 with g the host model's float32 curve:
    |z - z_ref| <= 1e-6 max|x| and |g - g_ref| <= 1e-6 (about four float32 roundings of a value in [0, 1], doubled: the division
    and the fused multiply-add differ).  In place equals out of place bit for bit; applied twice it is g^2 x to the same bound,
    forward being the adjoint."""
    x = rt.Ragged.from_list(clips)
    assert x.offsets[1] % 4 == 3
    seeds = [7, 0xFFFFFFFF, 123456789, 0]
    worst = [0.0, 0.0]
    for step, entry in ((0, 0), (3, 2)):
        z, g = rt.gain_envelope(x, seeds, step, entry, P, floor, return_gains=True)
        buf = rt.Ragged(x.data.clone(), x.lengths)
        same = rt.gain_envelope(buf, seeds, step, entry, (P, P), floor, out=buf)
        assert same is buf and torch.equal(buf.data, z.data)
        twice = rt.gain_envelope(z, seeds, step, entry, P, floor).to_list()
        for b, (xi, zi, gi, z2) in enumerate(zip(clips, z.to_list(), g.to_list(), twice)):
            r = LA.entry_draw(seeds[b], step, entry)
            Pd, ph = LA.envelope_draw({"period": [(P + 0.5) / 16000.0] * 2}, r, 16000)
            assert Pd == P and 0 <= ph < P
            gref = LA.envelope_curve(len(xi), seeds[b], step, entry, P, ph, floor).astype(np.float64)
            peak = float(np.abs(xi).max())
            eg = float(np.abs(gi - gref).max())
            ez = float(np.abs(zi - xi.astype(np.float64) * gref).max()) / peak
            e2 = float(np.abs(z2 - xi.astype(np.float64) * gref * gref).max()) / peak
            worst = [max(worst[0], eg), max(worst[1], ez, e2)]
            assert eg <= 1e-6 and ez <= 1e-6 and e2 <= 1e-6, (P, floor, step, entry, b, eg, ez, e2)
            assert float(gi.min()) >= floor - 1e-6 and float(gi.max()) <= 1.0
    print(f"gain_envelope P = {P}, floor = {floor}: max |g - model| = {worst[0]:.2e}, max |z - model| / peak = {worst[1]:.2e}")


def test_gain_envelope_draws_a_period_and_refuses_bad_arguments(rt, LA, clips):
    x = rt.Ragged.from_list(clips)
    seeds = [1, 2, 3, 4]
    z = rt.gain_envelope(x, seeds, 5, 1, (800, 8000), 0.0).to_list()
    entry = LA.parse_chain([ENV])[0]
    periods = set()
    for b, (xi, zi) in enumerate(zip(clips, z)):
        P, ph = LA.envelope_draw(entry, LA.entry_draw(seeds[b], 5, 1), 16000)
        periods.add(P)
        ref = xi.astype(np.float64) * LA.envelope_curve(len(xi), seeds[b], 5, 1, P, ph, 0.0)
        assert float(np.abs(zi - ref).max()) <= 1e-6 * float(np.abs(xi).max())
    assert len(periods) == 4
    for bad in (dict(period_samples=63), dict(period_samples=(800, 799)), dict(period_samples=(64, (1 << 20) + 1)), dict(floor=1.0),
                dict(floor=-0.1), dict(floor=float("nan")), dict(step=-1), dict(entry=4), dict(entry=-1)):
        kw = dict(dict(step=0, entry=0, period_samples=800, floor=0.0), **bad)
        with pytest.raises(ValueError):
            rt.gain_envelope(x, seeds, kw["step"], kw["entry"], kw["period_samples"], kw["floor"])
    with pytest.raises(ValueError):
        rt.gain_envelope(x, seeds[:3], 0, 0, 800)
    from aware_amd._lib import load_library
    lib = load_library()
    p = lambda t: C.c_void_p(t.data_ptr())
    sd = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.empty_like(x.data)
    args = lambda B=4, max_len=x.max_len, p_lo=64, p_hi=800, floor=0.0: (p(x.data), p(x.d_off), p(x.d_len), B, max_len, p(sd), 0, 0,
                                                                          p_lo, p_hi, floor, p(out), None, None)
    assert lib.aware_gain_envelope(*args(B=0)) == -1 and lib.aware_gain_envelope(*args(max_len=0)) == -1
    assert lib.aware_gain_envelope(*args(p_lo=63)) == -1 and lib.aware_gain_envelope(*args(p_hi=63)) == -1
    assert lib.aware_gain_envelope(*args(floor=1.0)) == -1
    assert lib.aware_gain_envelope(*args()) == 0
    torch.cuda.synchronize()


def test_the_attack_is_the_loops_first_step(rt, LA, clips):
    """attacks.GainEnvelope is the loop's envelope at step 0, entry 0, the convention of attacks.Reverberation; Fade and Tremolo are
    plain torch on the ragged buffer."""
    from aware_amd import attacks as A
    x = rt.Ragged.from_list(clips)
    atk = A.GainEnvelope(period=0.05, floor=0.25, seed=40)
    out = atk.apply_batch(x, 16000)
    assert torch.equal(out.data, rt.gain_envelope(x, [40, 41, 42, 43], 0, 0, 800, 0.25).data)
    np.testing.assert_array_equal(A.GainEnvelope(period=0.05, floor=0.25, seed=41).apply(clips[1], 16000), out.to_list()[1])
    z = LA.apply_chain([torch.from_numpy(clips[0]).double()], [{"kind": "gain_envelope", "period": 0.05, "floor": 0.25}], [40], 0)[0]
    assert float((torch.from_numpy(out.to_list()[0]).double() - z).abs().max()) <= 1e-6 * float(np.abs(clips[0]).max())
    n = LENGTHS[1]
    t = np.arange(n, dtype=np.float64)
    fin = A.Fade(seconds_in=None).apply_batch(x, 16000).to_list()[1]
    np.testing.assert_allclose(fin, clips[1] * (t / n), rtol=0, atol=1e-6)
    fout = A.Fade(seconds_out=None).apply_batch(x, 16000).to_list()[1]
    np.testing.assert_allclose(fout, clips[1] * ((n - 1 - t) / n), rtol=0, atol=1e-6)
    tr = A.Tremolo(4.0, 0.9).apply_batch(x, 16000).to_list()[1]
    np.testing.assert_allclose(tr, clips[1] * (1 - 0.45 * (1 + np.sin(2 * np.pi * 4.0 * t / 16000.0))), rtol=0, atol=2e-6)


# ---- 2. the stage kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CHAINS))
@pytest.mark.parametrize("lengths", [RAGGED, UNIFORM], ids=["ragged", "uniform32"])
def test_forward_matches_the_restatement(rt, O, LA, lengths, name):
    """Buffer 12 against apply_chain(N(N(buffer 9))) in float64 at steps 0, 1 and 2, by the check and the bound of the kinds the
    chain holds beside the envelope: test_gpu_loop_attacks.check_forward (1e-6 of a unit-peak signal, zeros where the restatement
    has them) for noise and suppression, test_gpu_loop_reverb.check_forward (CHAIN_BOUND of the peak, the responses) with a
    reverberation.  The envelopes (prob 0.75, periods drawn in 0.05-0.5 s) fire on some clips and steps and idle on others."""
    chain = CHAINS[name]
    seeds = [11 + 3 * i for i in range(len(lengths))]
    sess, batch, _, _ = session(rt, O, lengths, list(range(20, 20 + len(lengths))), chain, seeds, num_iterations=4)
    fired = [LA.fires(LA.entry_draw(s, step, 0)[0], chain[0].get("prob", 1.0)) for s in seeds for step in range(3)]
    assert name == "suppression_envelope" or any(fired) != (name == "envelope_prob_0")
    assert name == "suppression_envelope" or name == "envelope_prob_0" or not all(fired)

    def check(step):
        if name == "envelope_reverb_envelope":
            check_forward_reverb(rt, LA, sess, batch, chain, seeds, step, name)
        else:
            check_forward_01(LA, sess, batch, chain, seeds, step, name)

    sess.gradient()
    check(0)
    sess.iterate(2)
    check(1)
    sess.iterate(1)
    assert int(sess.step.cpu()[0]) == 3
    check(2)
    if name == "envelope_prob_0":
        for z, y in zip(attacked(sess, batch), synthesis(sess, batch)):
            assert float((z.double() - norm2(y.double())).abs().max()) < 2e-7


@pytest.mark.parametrize("name", list(CHAINS))
@pytest.mark.parametrize("lengths", [RAGGED, UNIFORM], ids=["ragged", "uniform32"])
def test_first_gradient(rt, O, LA, lengths, name):
    """aware_embed_gradient with the chain against torch autograd over the restatement composed with the oracle's loop body, by
    loop_support.check_first_gradient: 2e-5 relative L2 per clip (2e-2 within 2e-6 of a LeakyReLU kink), loss and
    prediction 1e-5."""
    check_first_gradient(rt, O, LA, CHAINS[name], lengths)


@pytest.mark.parametrize("kw", [dict(conv_pipe="f32"), dict(conv_pipe="bf16x3"), dict(conv_pipe="f16x2"),
                                dict(dsp_path="staged", mel="dense", conv_pipe="f32")],
                         ids=["f32", "bf16x3", "f16x2", "staged_dense_f32"])
def test_first_gradient_on_every_conv_pipe(rt, O, LA, kw):
    check_first_gradient(rt, O, LA, CHAINS["envelope_reverb_envelope"], RAGGED, **kw)
    check_first_gradient(rt, O, LA, [dict(ENV, prob=1.0), NOISE10], RAGGED, **kw)


# ---- 3. graph replay ----------------------------------------------------------------------------------------------------------
def test_graph_replay_is_bit_identical_and_redraws(rt, O):
    chain = [dict(ENV_SHORT, floor=0.0), NOISE10, dict(ENV, prob=1.0)]
    out, _ = graph_replay_bits(rt, O, chain, RAGGED, first=24)
    zs = out[4]
    for i in range(7):
        assert float((zs[i + 1] - zs[i]).abs().max()) > 1e-2        # the draw is keyed by the device step counter


def test_consecutive_steps_draw_different_envelopes(rt, O, LA):
    """Without noise the envelope is the ratio z / x: at steps 0 and 1 it is the host model's curve of that step, and the two differ."""
    chain = [{"kind": "gain_envelope", "period": 0.05, "floor": 0.25}]
    seeds = [3, 4, 5]
    sess, batch, _, _ = session(rt, O, RAGGED, [53, 54, 55], chain, seeds, num_iterations=4)
    curves = []
    for step in (0, 1):
        sess.iterate(1)
        torch.cuda.synchronize()
        per_clip = []
        for b, (y, z) in enumerate(zip(synthesis(sess, batch), attacked(sess, batch))):
            x = norm2(y.double())
            P, ph = LA.envelope_draw(LA.parse_chain(chain)[0], LA.entry_draw(seeds[b], step, 0), 16000)
            g = LA.envelope_curve(len(x), seeds[b], step, 0, P, ph, 0.25).astype(np.float64)
            assert float((z.double() - x * torch.from_numpy(g)).abs().max()) < 1e-6
            per_clip.append(g)
        curves.append(per_clip)
    for g0, g1 in zip(*curves):
        assert float(np.abs(g0 - g1).max()) > 0.2


# ---- 4. a mixture -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0.5, 0.3], ids=["no_clean_share", "clean_share"])
def test_a_mixture_with_an_envelope_chain(rt, O, LA, w):
    """[{w, [envelope]}, {w, [suppression, noise]}]: at steps 0, 2 and 5 every clip's z is that of the chain it drew
    (runtime.loop_mixture_draw is the host's mixture_choices), by test_gpu_loop_mixture.check_forward; with w = 0.3 the clips that
    drew neither are plain (within 2e-7 of N(N(y)))."""
    mixture = LA.parse_mixture([{"weight": w, "chain": [dict(ENV, prob=1.0)]}, {"weight": w, "chain": [SUP, NOISE10]}])
    lengths = [16000, 8000, 24000, 23456, 12001, 16000, 9000, 31999, 16384, 20000]
    want = {0, 1} | ({-1} if w < 0.5 else set())
    s0 = 100
    while set(LA.mixture_choices(range(s0, s0 + 10), 0, weights(mixture)).tolist()) != want:
        s0 += 1
    seeds = list(range(s0, s0 + 10))
    sess, batch = mixture_session(rt, O, lengths, seeds, mixture=mixture, num_iterations=8)
    sess.gradient()
    for step, more in ((0, 3), (2, 3), (5, 0)):
        np.testing.assert_array_equal(rt.loop_mixture_draw(seeds, step, weights(mixture)).cpu().numpy(),
                                      LA.mixture_choices(seeds, step, weights(mixture)))
        check_forward_mixture(LA, sess, batch, mixture, seeds, step, f"envelope mixture w = {w}")
        sess.iterate(more)
    # against the chain alone: a clip that drew the envelope chain has the bits of a handle that holds only that chain
    mix, _ = mixture_session(rt, O, lengths, seeds, mixture=mixture, num_iterations=8)
    one, _ = mixture_session(rt, O, lengths, seeds, chain=mixture[0]["chain"], num_iterations=8)
    g, g1 = mix.gradient(), one.gradient()
    torch.cuda.synchronize()
    choice = LA.mixture_choices(seeds, 0, weights(mixture))
    for b in np.flatnonzero(choice == 0):
        span = slice(batch.out_offsets[b], batch.out_offsets[b] + batch.out_lengths[b])
        rows = slice(batch.frame_offsets[b], batch.frame_offsets[b + 1])
        assert torch.equal(mix.attacked[span], one.attacked[span]) and torch.equal(g[rows], g1[rows])


# ---- 5. error codes -----------------------------------------------------------------------------------------------------------
def test_entry_point_error_codes(rt, O, LA):
    from aware_amd._lib import LoopAttack
    lengths = [16000, 8000]
    sess, batch, _, _ = session(rt, O, lengths, [64, 65], None, num_iterations=4, use_graph=False)
    lib = sess.lib
    ex = ex_entries
    ev = (8, 0.75, [800.0, 8000.0, 0.0])
    nb_noise = lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex([(0, 1.0, [10.0])]), 1)
    assert lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex([ev]), 1) == nb_noise        # no new workspace
    assert nb_noise == lib.aware_embed_loop_attack_workspace_bytes(batch.h, 1)
    ws = torch.empty(nb_noise, dtype=torch.uint8, device="cuda")
    seeds = (C.c_uint32 * 2)(1, 2)

    def call(entries, n=None):
        return lib.aware_embed_set_loop_attacks_ex(sess.h, ex(entries), len(entries) if n is None else n, seeds,
                                                   C.c_void_p(ws.data_ptr()), nb_noise, None)

    old = (LoopAttack * 1)(LoopAttack(8, 800.0, 1.0))
    assert lib.aware_embed_set_loop_attacks(sess.h, old, 1, seeds, C.c_void_p(ws.data_ptr()), nb_noise, None) == -1     # the older entry
    nan = float("nan")
    for bad in ([63.0, 800.0, 0.0], [801.0, 800.0, 0.0], [800.0, 1048577.0, 0.0], [800.5, 900.0, 0.0], [nan, 800.0, 0.0],
                [800.0, 8000.0, 1.0], [800.0, 8000.0, -0.1], [800.0, 8000.0, nan]):
        assert call([(8, 1.0, bad)]) == -1, bad
    assert call([(8, 1.5, [800.0, 8000.0, 0.0])]) == -1 and call([(9, 1.0, [800.0, 8000.0, 0.0])]) == -1
    assert call([ev] * 5, n=5) == -1
    assert not lib.aware_embed_buffer(sess.h, 12)                       # nothing was set by a refused call
    assert call([ev] * 4) == 0 and call([(8, 1.0, [64.0, 1048576.0, 0.999])]) == 0
    with pytest.raises(ValueError, match="outside 64"):
        sess.set_loop_attacks([{"kind": "gain_envelope", "period": 0.001}], [1, 2])
    # after a locked step the chain stays
    chain = [{"kind": "gain_envelope", "period": 0.05, "floor": 0.25}]
    sess.set_loop_attacks(chain, [1, 2])
    sess.iterate(1)
    assert call([ev]) == -1 and call([], n=0) == -1
    with pytest.raises(ValueError):
        sess.set_loop_attacks([NOISE10], [1, 2])
    sess.iterate(1)
    check_forward_01(LA, sess, batch, chain, [1, 2], 1, "after the refused calls")


# ---- 6. the value claim on the device ---------------------------------------------------------------------------------------------
def test_value_claim_on_the_device(rt, O, tmp_path):
    """The CPU test's experiment on the device: four 1 s clips, seeds 0..3, 400 steps through AWAREEmbedder(loop_attacks=
    [gain_envelope(period 0.05-0.5 s, prob 0.75)]) and AWAREDetector; BER under attacks.Fade over the whole clip (in, out),
    attacks.Tremolo at 1, 4 and 20 Hz with depth 0.9, and the middle half ducked to 0.1 by a torch multiply.  Clean 0 % for both
    embeddings, the plain mean over the six at least 10 %, the aware mean at most half of it.  Measured: plain 32.5 / 35 / 36.25 /
    36.25 / 30 / 40 %, mean 35.00 %; aware 0 / 0 / 2.5 / 5 / 13.75 / 6.25 %, mean 4.58 %; clean 0 %; SNR 15.8 against 14.2 dB."""
    from aware_amd import attacks as A
    from test_loop_gain_host import AWARE_CHAIN, snr_db
    clips, bits, embed, ber = value_claim_setup(O, tmp_path)

    def duck(x):
        data = x.data.clone()
        for o, n in zip(x.offsets, x.lengths):
            data[o + n // 4: o + n - n // 4] *= 0.1
        return rt.Ragged(data, x.lengths)

    def table(det, ys):
        x = rt.Ragged.from_list(ys)
        out = {"fade-in": ber(det, A.Fade(seconds_in=None).apply_batch(x, 16000)),
               "fade-out": ber(det, A.Fade(seconds_out=None).apply_batch(x, 16000))}
        for hz in (1.0, 4.0, 20.0):
            out[f"tremolo {hz:g} Hz"] = ber(det, A.Tremolo(hz, 0.9).apply_batch(x, 16000))
        out["middle half ducked"] = ber(det, duck(x))
        return out

    y0, det = embed(None)
    y1, _ = embed(AWARE_CHAIN)
    c0, c1 = ber(det, y0), ber(det, y1)
    b0, b1 = table(det, y0), table(det, y1)
    for k in b0:
        print(f"device: {k:20s} plain {b0[k]:6.2f} %   envelope-aware {b1[k]:6.2f} %")
    m0, m1 = float(np.mean(list(b0.values()))), float(np.mean(list(b1.values())))
    snr = [snr_db([c / (np.abs(c).max() + 1e-8) for c in clips], np.stack([v / (np.abs(v).max() + 1e-8) for v in ys])) for ys in (y0, y1)]
    print(f"device: clean BER plain {c0:.2f} % / envelope-aware {c1:.2f} %; mean over the six: plain {m0:.2f} % / aware {m1:.2f} %; "
          f"SNR against the host: plain {snr[0]:.1f} dB / aware {snr[1]:.1f} dB")
    assert c0 == 0.0 and c1 == 0.0
    assert m0 >= 10.0
    assert m1 <= 0.5 * m0
