"""Speed change inside the embed loop and as an attack (EXTENSION) on the device: the Catmull-Rom resampling kernel of
csrc/loop_speed_kernels.hip and its gather-form adjoint, alone and inside the loop, against the float64 torch restatement
aware_amd/embedding/loop_attacks.py composed with the oracle's loop body.

Shapes: clips [8000] * 2 (7936 output samples), [16000] * 2 (15872, more than one synthesis run per clip) and the ragged
[16000, 8000]; stand-alone clips of 4099 and 7937 samples, packed back to back so that the second starts at an odd offset.

Run on the MI355X box:  python -m pytest tests/test_gpu_loop_speed.py -m gpu -q -s"""
import ctypes as C

import numpy as np
import pytest
import torch

from loop_support import CHAIN_BOUND, LA, LONG, NOISE10, O, RAGGED, RV, SHORT, SUP, ex_entries, first_gradient
from loop_support import forward_at_steps_0_2_17, graph_replay_bits, norm2, prob_0_is_the_plain_loop, rt, sampled, session
from loop_support import step_0_is_the_stand_alone_entry, value_claim_setup

pytestmark = pytest.mark.gpu

M_MIN, M_MAX = -13520, 17034                               # ceil / floor of 65536 (2^(-+400 / 1200) - 1)
M_MID = 3000
SPEED = {"kind": "speed_change", "cents": 200.0}
CHAINS = {"speed": [SPEED], "speed_noise": [SPEED, NOISE10], "suppression_speed": [SUP, SPEED]}

# Largest error of the stand-alone operator against the float64 restatement on the same f32 operands, as a fraction of each
# clip's reference peak.  Positions and fractions are integers, exact on both sides.  Each weight is a cubic in Horner form,
# at most four f32 roundings; the forward sums four products (four more roundings) whose absolute values add up to at most
# 1.25 times the input's peak: 8 * 2^-24 * 1.25 = 6e-7.  The adjoint sums up to seven products per output, and the weights
# that reach one output add up to at most 1.26 * 1.25: 11 * 2^-24 * 1.6 = 1.05e-6.  CAP is twice that, for a reference peak
# below the operand's; a larger error is a defect.  SPEED_BOUND is four times the largest value measured over the cases of
# the test (for input dependence): 1.42e-7 over the twelve cases, forward 1.10e-7 and adjoint 1.42e-7 at most.
CAP = 2e-6
SPEED_BOUND = 5.7e-7
CHAIN_CAP = 5e-6                                           # the reverberation's ceiling for the loop's attacked signal (its CAP)


def one_value(LA, m):
    """A speed_change entry whose range of cents holds the one offset m."""
    c = 1200.0 * np.log2(1.0 + m / 65536.0)
    e = LA.parse_chain([{"kind": "speed_change", "cents": [c - 0.001, c + 0.001]}])[0]
    assert LA.speed_range(e) == (m, m)
    return e


def drawn(LA, chain, seed, step):
    """The offset the chain's speed change draws for this clip at this step; 0 where it does not fire."""
    chain = LA.parse_chain(chain)
    j = [a["kind"] for a in chain].index("speed_change")
    r = LA.entry_draw(seed, step, j)
    return LA.speed_offset(r[3], *LA.speed_range(chain[j])) if LA.fires(r[0], chain[j]["prob"]) else 0


# ---- 1. the operator alone ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def alone():
    """Two odd-length clips and a gradient for each side, shared by the tests of the stand-alone entry."""
    rng = np.random.default_rng(17)
    lengths = [4099, 7937]
    xs = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    return lengths, xs


@pytest.mark.parametrize("m", [M_MIN, M_MAX, -1, 0, 1, M_MID])
@pytest.mark.parametrize("true_speed", [False, True], ids=["same_length", "true_speed"])
def test_speed_change_against_the_restatement(rt, LA, alone, m, true_speed):
    """aware_speed_change, forward and adjoint, against the float64 restatement (autograd for the adjoint) on the f32
    operands; the taps at sample 0, at the last sample, at the truncation point and across the 1024-sample workgroup
    boundaries are part of the whole-clip comparison and checked once more by index; the dot-product identity between the two
    directions.  The second clip starts at float offset 4099 on the input side and at an odd offset on the output side."""
    lengths, xs = alone
    out_len = [LA.speed_length(n, m) for n in lengths] if true_speed else lengths
    rng = np.random.default_rng(m % 1000)
    gs = [rng.standard_normal(n).astype(np.float32) for n in out_len]
    x = rt.Ragged.from_list(xs)
    z = rt.speed_change(x, m, out_lengths=out_len)
    assert z.lengths == out_len and x.offsets[1] % 4 == 3
    gx = rt.speed_change(rt.Ragged.from_list(gs), [m, m], adjoint=True, out_lengths=lengths)
    assert gx.lengths == lengths
    worst_f = worst_a = 0.0
    for xi, gi, zi, gxi, n, no in zip(xs, gs, z.to_list(), gx.to_list(), lengths, out_len):
        xt = torch.from_numpy(xi).double().requires_grad_(True)
        ref = LA.speed_change(xt, m, no)
        (ref * torch.from_numpy(gi).double()).sum().backward()
        ref, refg = ref.detach().numpy(), xt.grad.numpy()
        assert zi.shape == (no,) and gxi.shape == (n,)
        worst_f = max(worst_f, np.abs(zi - ref).max() / np.abs(ref).max())
        worst_a = max(worst_a, np.abs(gxi - refg).max() / np.abs(refg).max())
        live = min(no, LA.speed_length(n, m))
        for i in sorted(i for i in {0, 1, 1023, 1024, 1025, 4095, 4096, live - 2, live - 1, no - 1} if 0 <= i < no):
            assert abs(zi[i] - ref[i]) <= SPEED_BOUND * np.abs(ref).max(), (i, zi[i], ref[i])
        assert np.all(zi[live:] == 0.0)                                    # beyond the clip's end: exact zeros
        if m == 0:
            assert np.array_equal(zi.view(np.uint32), xi[:no].view(np.uint32))       # the identity, bit for bit
            assert np.array_equal(gxi.view(np.uint32), gi[:n].view(np.uint32))
        a, b = float(np.dot(zi.astype(np.float64), gi)), float(np.dot(xi.astype(np.float64), gxi))
        # each side's error vector is at most SPEED_BOUND * peak per sample, and a peak is at most sqrt(n) times the rms
        slack = SPEED_BOUND * np.sqrt(max(n, no)) * (np.linalg.norm(ref) * np.linalg.norm(gi) + np.linalg.norm(xi) * np.linalg.norm(refg))
        assert abs(a - b) <= slack, (a, b, slack)
    print(f"speed_change m = {m}, {'true-speed' if true_speed else 'same'} length: max error / peak forward {worst_f:.2e}, "
          f"adjoint {worst_a:.2e}")
    assert worst_f < SPEED_BOUND <= CAP and worst_a < SPEED_BOUND, (worst_f, worst_a)


def test_speed_change_per_clip_offsets_and_errors(rt, LA, alone):
    lengths, xs = alone
    x = rt.Ragged.from_list(xs)
    # one offset per clip; a clip alone gives the same bits as inside a batch, wherever it starts
    z = rt.speed_change(x, [M_MID, -777]).to_list()
    for xi, zi, m in zip(xs, z, (M_MID, -777)):
        np.testing.assert_array_equal(rt.speed_change(rt.Ragged.from_list([xi]), [m]).to_list()[0], zi)
    from aware_amd import attacks as A
    atk = A.SpeedChange(cents=-84.0)
    out = atk.apply_batch(x, 16000)
    assert out.lengths == [LA.speed_length(n, atk.m) for n in lengths] and out.lengths[0] > lengths[0]
    np.testing.assert_array_equal(out.to_list()[1], rt.speed_change(x, atk.m, out_lengths=out.lengths).to_list()[1])
    np.testing.assert_array_equal(atk.apply(xs[0], 16000), out.to_list()[0])
    assert A.SpeedChange(cents=84.0).apply_batch(x, 16000).lengths[0] < lengths[0]
    for bad in ([1], [0, M_MAX + 1], [M_MIN - 1, 0]):
        with pytest.raises(ValueError):
            rt.speed_change(x, bad)
    with pytest.raises(ValueError):
        rt.speed_change(x, 0, out_lengths=[4099])
    with pytest.raises(ValueError):
        rt.speed_change(x, 0, out_lengths=[4099, 0])


# ---- 2. forward inside the loop -----------------------------------------------------------------------------------------------
def check_forward(LA, sess, batch, chain, seeds, step, tag, sample=None):
    torch.cuda.synchronize()
    worst = 0.0
    for b, y, z in sampled(sess, batch, sample):
        ref = LA.apply_chain(norm2(y.double())[None], chain, [seeds[b]], step)[0]
        worst = max(worst, float((z.double() - ref).abs().max() / ref.abs().max()))
        m = drawn(LA, chain, seeds[b], step)
        if m > 0 and chain[-1]["kind"] != "gaussian_noise":
            assert float(z[LA.speed_length(len(y), m):].abs().max()) == 0.0      # a faster clip ends in exact zeros
    print(f"{tag}, step {step}: max |z - restatement| / peak = {worst:.2e}")
    assert worst < CHAIN_BOUND <= CHAIN_CAP, (tag, step, worst)
    return worst


@pytest.mark.parametrize("name", list(CHAINS))
@pytest.mark.parametrize("lengths", [SHORT, LONG, RAGGED], ids=["short", "long", "ragged"])
def test_forward_matches_the_restatement(rt, O, LA, lengths, name):
    """Buffer 12 against apply_chain(N(N(buffer 9))) at steps 0, 2 and 17, within the bound of the reverberation's
    corresponding test (1.13e-6 of the peak).  Measured: 1.57e-7 at most over the 81 comparisons."""
    chain = LA.parse_chain(CHAINS[name])
    batch, seeds = forward_at_steps_0_2_17(rt, O, LA, chain, lengths, name, check_forward)
    assert len({drawn(LA, chain, seeds[0], s) for s in (0, 2, 17)}) == 3


@pytest.mark.parametrize("m", [M_MIN, M_MID, M_MAX])
@pytest.mark.parametrize("lengths", [LONG, RAGGED], ids=["long", "ragged"])
def test_step_0_is_the_stand_alone_entry(rt, O, LA, lengths, m):
    """With a range that holds one offset, buffer 12 at step 0 is aware_speed_change on the same input, bit for bit: the loop's
    kernel and the stand-alone one share their arithmetic.  The input x = N(N(y)) in the device's own rounding is buffer 12
    of a second session whose entry never fires."""
    step_0_is_the_stand_alone_entry(rt, O, lengths, one_value(LA, m), lambda x: rt.speed_change(x, m))


# ---- 3. first gradient ----------------------------------------------------------------------------------------------------------
# First clip seed of each gradient case, chosen on the CPU so that the float64 restatement keeps every LeakyReLU argument of
# every clip at least 1e-5 from its kink (speed 1.7e-5 / 1.3e-5, speed_noise 1.6e-5 / 3.1e-5, suppression_speed 1.3e-5 / 1.0e-4,
# the three entries 3.8e-5 / 1.9e-5 / 1.0e-5; from seed 40 on, speed_noise had a clip at 2.5e-7 and suppression_speed one at
# 9.9e-7).  The check below still allows one clip per case within KINK at 2e-2, and prints the distances.
KINK = 1e-6
SEED0 = {"speed": 83, "speed_noise": 80, "suppression_speed": 86, "three": 83}


def check_first_gradient(rt, O, LA, chain, lengths, clip_seed0, **kw):
    _, seeds, figures = first_gradient(rt, O, LA, chain, lengths, list(range(clip_seed0, clip_seed0 + len(lengths))), **kw)
    near = 0
    for i, (rel, kink, lerr, perr) in enumerate(figures):
        near += int(kink <= KINK)
        print(f"{kw} clip {i} (n = {lengths[i]}, m = {drawn(LA, chain, seeds[i], 0)}): loss err {lerr:.1e}, pred err {perr:.1e}, "
              f"gradient rel L2 {rel:.2e}, nearest LeakyReLU kink {kink:.1e}")
        assert lerr < 1e-5 and perr < 1e-5, (i, lerr, perr)
        assert rel < (2e-5 if kink > KINK else 2e-2), (i, rel, kink)
    assert near <= 1, near


@pytest.mark.parametrize("name", list(CHAINS))
@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
def test_first_gradient(rt, O, LA, name, dsp_path):
    """aware_embed_gradient against torch autograd over the restatement composed with the oracle's loop body: 2e-5 relative L2
    per clip (2e-2 for at most one clip per case with a LeakyReLU argument within 1e-6 of its kink), loss and prediction 1e-5.
    Measured over the gradient tests of this file: 3.6e-6 relative L2 at most, loss 2.4e-7, prediction 3.6e-7;
    no clip closer than 8e-6 to a kink."""
    check_first_gradient(rt, O, LA, CHAINS[name], RAGGED, SEED0[name], dsp_path=dsp_path)


@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
def test_first_gradient_three_entries(rt, O, LA, dsp_path):
    check_first_gradient(rt, O, LA, [SUP, dict(SPEED, cents=[-400.0, 400.0]), NOISE10], [8000, 16000, 24000], SEED0["three"],
                         dsp_path=dsp_path)


def test_first_gradient_f32_dense(rt, O, LA):
    check_first_gradient(rt, O, LA, CHAINS["speed_noise"], RAGGED, SEED0["speed_noise"], conv_pipe="f32", mel="dense")


# ---- 4. graph replay, prob 0, the older kinds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", [LONG, RAGGED], ids=["long", "ragged"])
def test_graph_replay_is_bit_identical_and_redraws(rt, O, LA, lengths):
    chain = [dict(SPEED, prob=0.75), NOISE10]
    out, batch = graph_replay_bits(rt, O, chain, lengths)
    # the draw is keyed by the device step counter: clip 0 (seed 0) at steps 32..39 is resampled at the offsets the host draws
    ms = [drawn(LA, chain, 0, s) for s in range(32, 40)]
    assert len(set(ms)) >= 6, ms
    n0 = batch.out_lengths[0]
    for i, m in enumerate(ms):
        z = out[4][i, :n0]
        live = LA.speed_length(n0, m)
        if m > 0:
            # behind a faster clip's end there is nothing but the noise entry's draw: far below the signal's level
            assert float(z[live:].abs().max()) < 2.0 and float(z[live:].std()) < float(z[:live].std())


def test_prob_0_is_the_plain_loop(rt, O):
    """A speed change that never fires against the loop without a chain: coefficients, best coefficients and losses after 20
    steps and the gradient of step 20, bit for bit, alone and between two older entries that never fire either, on both
    dsp_paths (a clip on which no entry fires takes the plain loop's path, as in chains with a reverberation)."""
    prob_0_is_the_plain_loop(rt, O, ([dict(SPEED, prob=0.0)], [dict(SUP, prob=0.0), dict(SPEED, prob=0.0), dict(NOISE10, prob=0.0)]))


def test_partly_idle_clips_and_older_kinds_keep_their_bits(rt, O, LA):
    """Two sessions built the same way agree bit for bit, for a chain of the three older kinds (through the _ex entry point, as
    before) and for one with a speed change that fires on some clips and steps only."""
    lengths = [16000, 8000, 24000]
    older = [dict(SUP, prob=0.75), {"kind": "reverberation", "rt60": [0.1, 0.3], "prob": 0.75}, NOISE10]
    for chain in (older, [dict(SUP, prob=0.5), dict(SPEED, prob=0.5)]):
        got = []
        for _ in range(2):
            sess, batch, _, _ = session(rt, O, lengths, [70, 71, 72], chain, [1, 2, 3], num_iterations=20)
            sess.iterate(20)
            g = sess.gradient()
            torch.cuda.synchronize()
            got.append((sess.coef.cpu(), sess.best_coef.cpu(), sess.loss.cpu(), sess.best_loss.cpu(), sess.attacked.cpu(), g.cpu()))
        for a, b in zip(*got):
            assert torch.equal(a, b)
    # every pattern of firing occurred among the 3 x 21 (clip, step) pairs of the second chain
    chain = LA.parse_chain([dict(SUP, prob=0.5), dict(SPEED, prob=0.5)])
    seen = {tuple(LA.fires(LA.entry_draw(sd, s, j)[0], 0.5) for j in range(2)) for sd in (1, 2, 3) for s in range(21)}
    assert len(seen) == 4


def test_entry_point_error_codes(rt, O):
    from aware_amd._lib import LoopAttack
    lengths = [16000, 8000]
    sess, batch, _, _ = session(rt, O, lengths, [64, 65], None, num_iterations=20, use_graph=False)
    lib = sess.lib
    ex, rv = ex_entries, RV
    sp = (3, 0.75, [-7150.0, 8025.0])
    nb_old = lib.aware_embed_loop_attack_workspace_bytes(batch.h, 1)
    nb0 = lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex([(0, 1.0, [10.0]), (1, 1.0, [4800.0])]), 2)
    nb_rv = lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex([rv]), 1)
    nb = lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex([(0, 1.0, [10.0]), sp]), 2)
    assert nb0 == nb_old                                                   # the older kinds need what they needed
    assert nb_old + 4 * batch.total_out <= nb < nb_old + 4 * batch.total_out + 256 and nb < nb_rv      # the one signal u
    assert lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex([sp]), 0) == 0
    ws = torch.empty(nb_rv, dtype=torch.uint8, device="cuda")
    seeds = (C.c_uint32 * 2)(1, 2)

    def call(entries, n=None, wsb=nb, sd=seeds):
        return lib.aware_embed_set_loop_attacks_ex(sess.h, ex(entries), len(entries) if n is None else n, sd,
                                                   C.c_void_p(ws.data_ptr()), wsb, None)

    old = (LoopAttack * 1)(LoopAttack(3, 0.0, 1.0))
    assert lib.aware_embed_set_loop_attacks(sess.h, old, 1, seeds, C.c_void_p(ws.data_ptr()), nb, None) == -1     # stays refused
    assert call([(3, 1.0, [0.5, 8025.0])]) == -1 and call([(3, 1.0, [-7150.0, 8024.5])]) == -1      # not integers
    assert call([(3, 1.0, [10.0, 0.0])]) == -1 and call([(3, 1.0, [1.0, 0.0])]) == -1               # m_lo > m_hi
    assert call([(3, 1.0, [float(M_MIN - 1), 0.0])]) == -1 and call([(3, 1.0, [0.0, float(M_MAX + 1)])]) == -1
    assert call([(3, 1.0, [float("nan"), 0.0])]) == -1 and call([(3, 1.0, [0.0, float("inf")])]) == -1
    assert call([(3, 1.5, [0.0, 0.0])]) == -1
    assert call([sp, (3, 1.0, [0.0, 0.0])]) == -1                                                   # a second speed change
    assert call([sp, rv], wsb=nb_rv) == -1 and call([rv, (0, 1.0, [10.0]), sp], wsb=nb_rv) == -1    # beside a reverberation
    assert call([sp], n=5) == -1 and call([sp], sd=None) == -1
    assert call([sp], wsb=nb - 256) == -4
    assert call([(3, 1.0, [float(M_MIN), float(M_MAX)])]) == 0
    assert call([(3, 1.0, [0.0, 0.0])]) == 0
    assert call([sp]) == 0 and lib.aware_embed_buffer(sess.h, 12) and not lib.aware_embed_buffer(sess.h, 13)
    assert call([], n=0) == 0 and not lib.aware_embed_buffer(sess.h, 12)
    assert call([(0, 1.0, [10.0]), sp]) == 0
    sess.iterate(1)
    torch.cuda.synchronize()
    assert call([sp]) == -1 and call([], n=0) == -1                        # after the first iterate
    with pytest.raises(ValueError):
        sess.set_loop_attacks([SPEED], [1, 2])


# ---- 5. the value claim on the device ---------------------------------------------------------------------------------------------
def test_value_claim_on_the_device(rt, O, tmp_path):
    """Four 1 s clips, seeds 0..3, 400 steps through AWAREEmbedder(loop_attacks=...) from an edited card: clean BER 0 % for both
    embeddings; under the polyphase resampler (attacks.resample_poly_batch) at 21/20, 20/21, 11/10 and 10/11 the plain BER is
    at least 25 % in the mean and the speed-aware one at most a third of it.  Measured: clean 0 % both;
    101/100 16.25 % plain against 0 %, 100/101 21.25 / 1.25, 21/20 40.00 / 3.75, 20/21 46.25 / 12.50, 11/10 61.25 / 8.75, 10/11
    46.25 / 20.00; mean of the last four 48.44 % against 11.25 %.  SNR against the normalised host: plain 15.93, 15.12, 15.88,
    16.08 dB; speed-aware 15.66, 15.84, 16.18, 15.53 dB."""
    from aware_amd import attacks as A
    from test_loop_speed_host import AWARE_CHAIN, RATIOS, snr_db
    clips, bits, embed, ber = value_claim_setup(O, tmp_path)

    y0, det = embed(None)
    y1, _ = embed(AWARE_CHAIN)
    c0, c1 = ber(det, y0), ber(det, y1)
    print(f"clean BER: plain {c0:.2f} %, speed-aware {c1:.2f} %")
    r0, r1 = [], []
    for up, down in [(101, 100), (100, 101)] + RATIOS:
        b0 = ber(det, A.resample_poly_batch(rt.Ragged.from_list(y0), up, down))
        b1 = ber(det, A.resample_poly_batch(rt.Ragged.from_list(y1), up, down))
        print(f"polyphase {up}/{down} ({1200 * np.log2(down / up):+.0f} cents): plain {b0:.2f} %, speed-aware {b1:.2f} %")
        if (up, down) in RATIOS:
            r0.append(b0)
            r1.append(b1)
    m0, m1 = float(np.mean(r0)), float(np.mean(r1))
    print(f"mean of the four wide ratios: plain {m0:.2f} %, speed-aware {m1:.2f} %")
    audio = np.stack(clips)
    print("SNR against the normalised host, dB: plain " + ", ".join(f"{v:.2f}" for v in snr_db(np.stack(y0), audio))
          + " / speed-aware " + ", ".join(f"{v:.2f}" for v in snr_db(np.stack(y1), audio)))
    assert c0 == 0.0 and c1 == 0.0
    assert m0 >= 25.0
    assert m1 <= m0 / 3.0
