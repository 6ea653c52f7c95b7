"""Reverberation inside the embed loop and as an attack (EXTENSION) on the device: the impulse-response and partitioned FFT
convolution kernels of csrc/loop_reverb_kernels.hip, alone and inside the loop, against float64 numpy and the torch restatement
aware_amd/embedding/loop_attacks.py composed with the oracle's loop body.

Shapes: clips [8000] * 4 (7936 output samples, fewer than an 8192-tap response) and the ragged [8000, 16000, 40000]; responses
of 600, 2048, 2049 and 8192 taps (one partition, exactly one, one tap more, all four).

Run on the MI355X box:  python -m pytest tests/test_gpu_loop_reverb.py -m gpu -q -s"""
import ctypes as C

import numpy as np
import pytest
import torch

from loop_support import CHAIN_BOUND, LA, NOISE10, O, RV, SUP, attacked, check_first_gradient, ex_entries, graph_replay_bits
from loop_support import norm2, prob_0_is_the_plain_loop, rt, sampled, session, synthesis, value_claim_setup

pytestmark = pytest.mark.gpu

# rt60 in seconds -> taps at 16 kHz; every test that uses one asserts int(rt60 * 16000)
RT60 = {600: 0.0375, 2048: 0.128, 2049: 0.12807, 8192: 0.512}
UNIFORM, RAGGED = [8000] * 4, [8000, 16000, 40000]

# Largest error of the device against the float64 reference as a fraction of each clip's reference peak: four times the
# largest value measured over the cases of the test (for input dependence), and never above CAP = 5e-6 -- 1.6e-7 per rfft and
# 3e-7 per irfft of the largest magnitude, two forward transforms, four partitions, one inverse: a
# larger error is a defect.  Measured: 2.99e-7 over the twelve cases of the convolution alone (forward and adjoint), 2.81e-7
# over the ninety comparisons of buffer 12 with the restatement.
CAP = 5e-6
CONV_BOUND = 1.2e-6
assert CHAIN_BOUND == 1.13e-6                              # four times the 2.81e-7 above, rounded; held by every later kind as well
# The device draws its normals in f32: each within 8 ulp of its magnitude (log, sqrt, sincospi and a product; the largest of
# 8192 draws is below 5.5: 8 * 2^-23 * 5.5 = 5.2e-6), under an envelope <= 1.  The direct path is a root of their sum of
# squares (f64, fixed order): at worst all 8 ulp one way, and the rounding of the result to f32.
IR_TAIL = 5.2e-6            # absolute
IR_DIRECT = 8 * 2.0 ** -23 + 2.0 ** -24      # relative


def ir_errors(h, ref):
    return float(np.abs(h[1:] - ref[1:]).max()) if len(ref) > 1 else 0.0, abs(float(h[0]) / ref[0] - 1.0)


def reverb(taps=None, **kw):
    e = {"kind": "reverberation", "rt60": RT60[taps] if taps else [0.1, 0.5], "drr_db": -3.0}
    if taps:
        assert int(e["rt60"] * 16000) == taps
    e.update(kw)
    return e


def chains(taps=None, **kw):
    r = reverb(taps, **kw)
    return {"reverb": [r], "reverb_noise": [r, NOISE10], "suppression_reverb": [SUP, r]}


def responses(LA, seeds, step, entry, taps, drr=-3.0):
    return [LA.reverb_ir(s, step, entry, taps, drr) for s in seeds]


def upload(hs, stride=8192):
    h = np.zeros((len(hs), stride), dtype=np.float32)
    for i, v in enumerate(hs):
        h[i, :len(v)] = v
    return torch.from_numpy(h).cuda(), torch.tensor([len(v) for v in hs], dtype=torch.int32, device="cuda")


# ---- 1. the convolution alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps", [600, 2048, 2049, 8192])
@pytest.mark.parametrize("lengths", [[7936] * 4, [7936, 15872, 39936], [4097, 2048, 6145, 1]], ids=["uniform", "ragged", "odd"])
def test_convolve_against_numpy(rt, LA, lengths, taps):
    """aware_convolve, forward and adjoint, against float64 np.convolve / np.correlate of the f32 operands, and the dot-product
    identity <conv(x), g> = <x, corr(g)> between the two directions."""
    assert int(RT60[taps] * 16000) == taps
    rng = np.random.default_rng(taps)
    xs = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    gs = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    hs = [h.astype(np.float32) for h in responses(LA, range(7, 7 + len(lengths)), 3, 1, taps)]
    hd, nh = upload(hs, stride=8192 if taps > 2049 else 2560)
    y = rt.convolve(rt.Ragged.from_list(xs), hd, nh).to_list()
    c = rt.convolve(rt.Ragged.from_list(gs), hd, nh, adjoint=True).to_list()
    worst = 0.0
    for x, g, h, yi, ci in zip(xs, gs, hs, y, c):
        n = len(x)
        ref = np.convolve(x.astype(np.float64), h.astype(np.float64))[:n]
        refc = np.correlate(np.concatenate([g.astype(np.float64), np.zeros(len(h) - 1)]), h.astype(np.float64), mode="valid")
        assert yi.shape == (n,) and ci.shape == (n,) and refc.shape == (n,)
        worst = max(worst, np.abs(yi - ref).max() / np.abs(ref).max(), np.abs(ci - refc).max() / np.abs(refc).max())
        a, b = float(np.dot(yi.astype(np.float64), g)), float(np.dot(x.astype(np.float64), ci))
        # each side's error vector is at most CONV_BOUND * peak per sample, and a peak is at most sqrt(n) times the rms
        slack = CONV_BOUND * np.sqrt(n) * (np.linalg.norm(ref) * np.linalg.norm(g) + np.linalg.norm(x) * np.linalg.norm(refc))
        assert abs(a - b) <= slack, (a, b, slack)
    print(f"convolve {lengths} x {taps} taps: max error / peak = {worst:.2e}")
    assert worst < CONV_BOUND <= CAP, worst


def test_convolve_identity_in_place_and_errors(rt, LA):
    x = rt.Ragged.from_list([np.random.default_rng(1).standard_normal(n).astype(np.float32) for n in (7936, 4097)])
    hd, nh = upload([h.astype(np.float32) for h in responses(LA, [1, 2], 0, 0, 600)], stride=600)
    # nh = 0 copies the clip exactly, in both directions
    zero = torch.zeros_like(nh)
    assert torch.equal(rt.convolve(x, hd, zero).data, x.data) and torch.equal(rt.convolve(x, hd, zero, adjoint=True).data, x.data)
    # out may be in: the spectra are complete before the first output sample is written
    from aware_amd._lib import load_library
    lib = load_library()
    ref = rt.convolve(x, hd, nh)
    nbytes = lib.aware_convolve_workspace_bytes(x.B, x.max_len, sum(x.lengths), 600)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    buf = x.data.clone()
    args = lambda wsb, stride=600: (C.c_void_p(buf.data_ptr()), C.c_void_p(x.d_off.data_ptr()), C.c_void_p(x.d_len.data_ptr()), x.B,
                                    x.max_len, C.c_void_p(hd.data_ptr()), stride, C.c_void_p(nh.data_ptr()), 0,
                                    C.c_void_p(buf.data_ptr()), C.c_void_p(ws.data_ptr()), wsb, None)
    assert lib.aware_convolve(*args(nbytes - 1)) == -4
    assert lib.aware_convolve(*args(nbytes, stride=0)) == -1 and lib.aware_convolve(*args(nbytes, stride=8193)) == -1
    assert lib.aware_convolve(*args(nbytes)) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf, ref.data)
    with pytest.raises(ValueError):
        rt.convolve(x, hd[:1], nh)
    with pytest.raises(ValueError):
        rt.reverb_ir([1, 2], 0, 0, 600, 599, -3.0)
    with pytest.raises(ValueError):
        rt.reverb_ir([1, 2], 0, 0, 600, 8192, -3.0, stride=4096)


# ---- 2. the impulse responses ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_lo,n_hi", [(600, 600), (2048, 2049), (1600, 8000), (8192, 8192), (2, 3)])
def test_reverb_ir_against_the_restatement(rt, LA, n_lo, n_hi):
    seeds = [0, 1, 17, 0xFFFFFFFF, 123456789]
    worst = [0.0, 0.0]
    for step, entry, drr in ((0, 0, -3.0), (5, 2, 6.0), (399, 3, -12.5)):
        h, nh = rt.reverb_ir(seeds, step, entry, n_lo, n_hi, drr)
        h, nh = h.cpu().numpy(), nh.cpu().numpy()
        for b, s in enumerate(seeds):
            n = LA.reverb_length(LA.entry_draw(s, step, entry)[2], n_lo, n_hi)
            assert nh[b] == n and n_lo <= n <= n_hi
            ref = LA.reverb_ir(s, step, entry, n, drr)
            assert np.all(h[b, n:] == 0)
            worst = [max(w, e) for w, e in zip(worst, ir_errors(h[b, :n], ref))]
    print(f"reverb_ir [{n_lo}, {n_hi}]: tail max error {worst[0]:.2e}, direct path relative error {worst[1]:.2e}")
    assert worst[0] < IR_TAIL and worst[1] < IR_DIRECT


# ---- 3. forward inside the loop -----------------------------------------------------------------------------------------------
def check_forward(rt, LA, sess, batch, chain, seeds, step, tag, sample=None):
    torch.cuda.synchronize()
    j = [a["kind"] for a in chain].index("reverberation")
    entry = LA.parse_chain(chain)[j]
    hs = sess.impulse_responses.cpu().numpy()
    worst, worst_h = 0.0, [0.0, 0.0]
    for b, y, z in sampled(sess, batch, sample):
        r = LA.entry_draw(seeds[b], step, j)
        n_h = LA.reverb_length(r[2], *LA.reverb_taps(entry, 16000))
        if LA.fires(r[0], entry["prob"]):
            href = LA.reverb_ir(seeds[b], step, j, n_h, entry["drr_db"])
            assert np.all(hs[b, n_h:] == 0)
            worst_h = [max(w, e) for w, e in zip(worst_h, ir_errors(hs[b, :n_h], href))]
        else:
            assert hs[b, 0] == 1.0 and np.all(hs[b, 1:] == 0)
        ref = LA.apply_chain(norm2(y.double())[None], chain, [seeds[b]], step)[0]
        worst = max(worst, float((z.double() - ref).abs().max() / ref.abs().max()))
    print(f"{tag}, step {step}: max |z - restatement| / peak = {worst:.2e}, responses: tail {worst_h[0]:.2e}, direct {worst_h[1]:.2e}")
    assert worst_h[0] < IR_TAIL and worst_h[1] < IR_DIRECT, (tag, step, worst_h)
    assert worst < CHAIN_BOUND <= CAP, (tag, step, worst)


@pytest.mark.parametrize("taps", [600, 2048, 2049, 8192, None])
@pytest.mark.parametrize("name", ["reverb", "reverb_noise", "suppression_reverb"])
@pytest.mark.parametrize("lengths", [UNIFORM, RAGGED], ids=["uniform", "ragged"])
def test_forward_matches_the_restatement(rt, O, LA, lengths, name, taps):
    """Buffer 12 against apply_chain(N(N(buffer 9))) and buffer 13 against reverb_ir at steps 0, 2 and 17 (taps None: lengths
    drawn from rt60 0.1-0.5 s with prob 0.75, so some clips pass through)."""
    chain = chains(taps, **({} if taps else {"prob": 0.75}))[name]
    seeds = [11 + 3 * i for i in range(len(lengths))]
    sess, batch, _, _ = session(rt, O, lengths, list(range(20, 20 + len(lengths))), chain, seeds, num_iterations=20)
    assert batch.out_lengths[0] == 7936
    sess.gradient()
    check_forward(rt, LA, sess, batch, chain, seeds, 0, name)
    sess.iterate(3)
    check_forward(rt, LA, sess, batch, chain, seeds, 2, name)
    sess.iterate(15)
    assert int(sess.step.cpu()[0]) == 18
    check_forward(rt, LA, sess, batch, chain, seeds, 17, name)


@pytest.mark.parametrize("taps", [600, 2049, 8192])
@pytest.mark.parametrize("lengths", [UNIFORM, RAGGED], ids=["uniform", "ragged"])
def test_step_0_is_the_post_hoc_attack(rt, O, LA, lengths, taps):
    """At step 0 and chain index 0 the loop's reverberation is attacks.Reverberation of the same seeds on x = N(N(y)).  The two
    run the same kernels; x is rounded differently on the host (3e-7 of its unit peak per sample, as in
    test_gpu_loop_attacks), which the response spreads: 4 sigma of independent errors of that size through h."""
    from aware_amd import attacks as A
    seeds = [3 + i for i in range(len(lengths))]
    sess, batch, _, _ = session(rt, O, lengths, list(range(30, 30 + len(lengths))), [reverb(taps)], seeds)
    sess.gradient()
    torch.cuda.synchronize()
    xs = [norm2(y).float().numpy() for y in synthesis(sess, batch)]
    atk = A.Reverberation(rt60=RT60[taps], drr_db=-3.0)
    out = atk.apply_batch(rt.Ragged.from_list(xs), 16000, seeds=seeds).to_list()
    for b, (z, r) in enumerate(zip(attacked(sess, batch), out)):
        assert r.shape == z.shape
        h = LA.reverb_ir(seeds[b], 0, 0, taps, -3.0)
        bound = 2 * CONV_BOUND + 4 * 3e-7 * np.linalg.norm(h) / np.abs(r).max()
        err = np.abs(z.numpy().astype(np.float64) - r).max() / np.abs(r).max()
        print(f"clip {b}, {taps} taps: loop against attacks.Reverberation {err:.2e} (bound {bound:.2e})")
        assert err < bound
    # the default seeds are seed + i, and apply() is apply_batch of one clip
    a0 = A.Reverberation(rt60=RT60[taps], seed=seeds[0])
    np.testing.assert_array_equal(a0.apply_batch(rt.Ragged.from_list(xs), 16000).to_list()[1], out[1])
    np.testing.assert_array_equal(a0.apply(xs[0], 16000), out[0])


# ---- 4. first gradient ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["reverb", "reverb_noise", "suppression_reverb"])
@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
def test_first_gradient(rt, O, LA, name, dsp_path):
    """aware_embed_gradient against torch autograd over the restatement composed with the oracle's loop body: 2e-5 relative L2
    per clip (2e-2 for a clip with a LeakyReLU argument within 2e-6 of its kink), loss and prediction 1e-5.  An 8000-sample
    clip under a 2049-tap response and a longer one.  Measured over the gradient tests of this file: 3.2e-6 relative L2 at
    most away from a kink (5.6e-4 for the one clip 1e-7 from one), loss 2.4e-7, prediction 5.9e-7."""
    check_first_gradient(rt, O, LA, chains(2049)[name], [8000, 16000], dsp_path=dsp_path)


@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
def test_first_gradient_ragged(rt, O, LA, dsp_path):
    check_first_gradient(rt, O, LA, [SUP, reverb(8192), NOISE10], RAGGED, dsp_path=dsp_path)


def test_first_gradient_f32_dense(rt, O, LA):
    check_first_gradient(rt, O, LA, chains(600)["reverb_noise"], [8000, 16000], conv_pipe="f32", mel="dense")


# ---- 5. graph replay, prob 0, the older kinds through the new entry point ----------------------------------------------------------
@pytest.mark.parametrize("lengths", [UNIFORM, RAGGED], ids=["uniform", "ragged"])
def test_graph_replay_is_bit_identical_and_redraws(rt, O, lengths):
    chain = [reverb(None, prob=0.75), NOISE10]
    out, _ = graph_replay_bits(rt, O, chain, lengths, more=("impulse_responses",))
    hs = out[5]
    for i in range(7):
        assert float((hs[i + 1] - hs[i]).abs().max()) > 1e-2        # the draw is keyed by the device step counter


def test_prob_0_is_the_plain_loop(rt, O):
    """A reverberation that never fires against the loop without a chain: coefficients, best coefficients and losses after 20
    steps and the gradient of step 20, bit for bit, alone and between two older entries that never fire either, on both
    dsp_paths.  A clip on which no entry of a chain with a reverberation fires takes the plain loop's path: z is still
    N(N(y)) (buffer 12), its maxima are recorded as 1, so the analysis' normalisers are the identity, and the backward stages
    pass the synthesis adjoint's gradient, partial sums and reflect pads through.  (A first version ran the normalisers'
    backward twice for such a clip and differed from the plain loop by 9.2e-5 in the coefficients after 20 steps.)"""
    prob_0_is_the_plain_loop(rt, O, ([reverb(None, prob=0.0)], [dict(SUP, prob=0.0), reverb(8192, prob=0.0), dict(NOISE10, prob=0.0)]))


def test_entry_point_error_codes_and_old_kinds(rt, O):
    from aware_amd._lib import LoopAttack
    lengths = [16000, 8000]
    sess, batch, _, _ = session(rt, O, lengths, [64, 65], None, num_iterations=20, use_graph=False)
    lib = sess.lib
    ex, rv = ex_entries, RV
    nb_old = lib.aware_embed_loop_attack_workspace_bytes(batch.h, 1)
    nb0 = lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex([(0, 1.0, [10.0])]), 1)
    nb = lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex([rv]), 1)
    assert nb0 == nb_old                                                   # the older kinds need what they needed
    # one more signal, the responses, and the spectra: 4 partitions and ceil(15872 / 2048) = 8 blocks of 2056 complex per clip
    assert nb >= nb_old + 4 * batch.total_out + 2 * 4 * 8192 + 8 * 2056 * 2 * (4 + 8)
    assert lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex([rv]), 0) == 0
    assert lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex([rv]), 5) == 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    seeds = (C.c_uint32 * 2)(1, 2)

    def call(entries, n=None, wsb=nb, sd=seeds):
        return lib.aware_embed_set_loop_attacks_ex(sess.h, ex(entries), len(entries) if n is None else n, sd,
                                                   C.c_void_p(ws.data_ptr()), wsb, None)

    old = (LoopAttack * 1)(LoopAttack(2, 4800.0, 1.0))
    assert lib.aware_embed_set_loop_attacks(sess.h, old, 1, seeds, C.c_void_p(ws.data_ptr()), nb, None) == -1     # stays refused
    assert call([rv, (2, 1.0, [600.0, 600.0, -3.0])]) == -1               # two reverberations
    assert call([(2, 1.0, [1.0, 600.0, -3.0])]) == -1                     # n_lo < 2
    assert call([(2, 1.0, [600.0, 8193.0, -3.0])]) == -1                  # n_hi > 8192
    assert call([(2, 1.0, [601.0, 600.0, -3.0])]) == -1                   # n_lo > n_hi
    assert call([(2, 1.0, [600.5, 700.0, -3.0])]) == -1 and call([(2, 1.0, [600.0, 700.5, -3.0])]) == -1
    assert call([(2, 1.0, [600.0, 700.0, float("nan")])]) == -1 and call([(2, 1.0, [600.0, 700.0, float("inf")])]) == -1
    assert call([(2, 1.0, [float("nan"), 700.0, -3.0])]) == -1 and call([(2, 1.5, [600.0, 700.0, -3.0])]) == -1
    assert call([(3, 1.0, [10.0])]) == -1 and call([rv], n=5) == -1 and call([rv], sd=None) == -1
    assert call([rv], wsb=nb - 1) == -4
    assert call([(0, 1.0, [10.0])], wsb=nb_old) == 0 and not lib.aware_embed_buffer(sess.h, 13)
    assert call([(2, 1.0, [2.0, 8192.0, 0.0])]) == 0
    assert call([rv]) == 0 and lib.aware_embed_buffer(sess.h, 12) and lib.aware_embed_buffer(sess.h, 13)
    assert call([], n=0) == 0 and not lib.aware_embed_buffer(sess.h, 12) and not lib.aware_embed_buffer(sess.h, 13)
    with pytest.raises(ValueError, match="taps"):
        sess.set_loop_attacks([{"kind": "reverberation", "rt60": 0.6}], [1, 2])
    # kinds 0 and 1 through the new entry point: the bits of the old one
    chain = [dict(SUP, prob=0.75), NOISE10]
    ref, _, _, _ = session(rt, O, lengths, [64, 65], chain, [1, 2], num_iterations=20, use_graph=False)
    assert call([(1, 0.75, [4800.0]), (0, 1.0, [10.0])]) == 0
    ref.iterate(20)
    sess.iterate(20)
    torch.cuda.synchronize()
    zero_off = lib.aware_embed_buffer(sess.h, 12) - ws.data_ptr()
    z = ws[zero_off: zero_off + 4 * batch.total_out].view(torch.float32)
    assert torch.equal(z, ref.attacked) and torch.equal(sess.coef, ref.coef) and torch.equal(sess.loss, ref.loss)
    assert call([rv]) == -1 and call([], n=0) == -1                        # after the first iterate


# ---- 6. the value claim on the device ---------------------------------------------------------------------------------------------
def test_value_claim_on_the_device(rt, O, tmp_path):
    """Four 1 s clips, seeds 0..3, 400 steps through AWAREEmbedder(loop_attacks=...): clean BER 0 % for both embeddings; under
    three fixed responses of rt60 0.3 s from numpy's generator (the CPU test's) the plain BER is at least 10 % and the
    reverberation-aware one at most half of it; the same under the echo y[1600:] += 0.7 y[:-1600].  Measured: 40.42 % against 11.67 % under the
    responses, 30.00 % against 6.25 % under the echo, clean 0 % for both."""
    from test_loop_reverb_host import AWARE_CHAIN, room_response
    clips, bits, embed, ber = value_claim_setup(O, tmp_path)

    def rooms(det, ys):
        x = rt.Ragged.from_list(ys)
        return float(np.mean([ber(det, rt.convolve(x, *upload([room_response(s).astype(np.float32)] * 4, stride=4800)))
                              for s in range(3)]))

    def echo(det, ys):
        out = []
        for y in ys:
            z = y.astype(np.float64).copy()
            z[1600:] += 0.7 * y[:-1600]
            out.append(z.astype(np.float32))
        return ber(det, out)

    y0, det = embed(None)
    y1, _ = embed(AWARE_CHAIN)
    c0, c1 = ber(det, y0), ber(det, y1)
    r0, r1, e0, e1 = rooms(det, y0), rooms(det, y1), echo(det, y0), echo(det, y1)
    print(f"clean BER: plain {c0:.2f} %, reverberation-aware {c1:.2f} %")
    print(f"rt60 0.3 s: plain {r0:.2f} %, aware {r1:.2f} %;  echo 100 ms x 0.7: plain {e0:.2f} %, aware {e1:.2f} %")
    assert c0 == 0.0 and c1 == 0.0
    assert r0 >= 10.0 and r1 <= 0.5 * r0
    assert e0 >= 10.0 and e1 <= 0.5 * e0
