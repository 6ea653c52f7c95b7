"""Pitch shift inside the embed loop and as an attack (EXTENSION) on the device: the fused kernel of
csrc/loop_pitch_kernels.hip (overlap-add stretch at the coupled rate and resampling in one launch, the stretched signal in LDS
only) and its gather-form adjoint, alone and inside the loop, against the float64 torch restatement
aware_amd/embedding/loop_attacks.py composed with the oracle's loop body.

Shapes: clips [8000] * 2 (7936 output samples), [16000] * 2 (15872, more than one synthesis run per clip) and the ragged
[16000, 8000]; stand-alone clips of 4099 and 7937 samples, packed back to back so that the second starts at an odd offset.

Run on the MI355X box:  python -m pytest tests/test_gpu_loop_pitch.py -m gpu -q -s"""
import ctypes as C

import numpy as np
import pytest
import torch

from loop_support import CHAIN_BOUND, KINK, LA, LONG, NO, NOISE10, O, PS, RAGGED, RV, SHORT, SP, ST, SU, SUP, ex_entries
from loop_support import first_gradient, forward_at_steps_0_2_17, graph_replay_bits, norm2, older_chains_workspace
from loop_support import prob_0_is_the_plain_loop, rt, sampled, session, step_0_is_the_stand_alone_entry, value_claim_setup

pytestmark = pytest.mark.gpu

M_MIN, M_MAX = -13520, 17034                               # the speed offsets of -+400 cents
M_MID = 3000
PITCH = {"kind": "pitch_shift", "cents": 100.0}
CHAINS = {"pitch": [PITCH], "pitch_noise": [PITCH, NOISE10], "suppression_pitch": [SUP, PITCH]}
assert CHAIN_BOUND == 1.13e-6                              # the project's bound for the loop's attacked signal

# Largest error of the stand-alone operator against the float64 restatement on the same f32 operands, as a fraction of each
# clip's reference peak.  Positions, window indices and interpolation fractions are exact on both sides; the device rounds the
# stretch's four fused multiply-adds and its halving, then the four Horner weights and the four-term interpolation of those
# rounded samples, so the roundings of the two operators compose: CAP is the sum of their two ceilings of 2e-6, and a larger
# error is a defect.  PITCH_BOUND is four times the largest value measured on the MI355X over the cases of the test (for input
# dependence): 1.83e-7 over the twelve cases, forward 1.83e-7 (at m = -13520) and adjoint 1.60e-7 (at m = -1) at most.
CAP = 4e-6
PITCH_BOUND = 7.3e-7


def one_value(LA, m):
    """A pitch_shift entry whose range of cents holds the one speed offset m."""
    lo, hi = 1200.0 * np.log2(1.0 + (m - 0.5) / 65536.0), 1200.0 * np.log2(1.0 + (m + 0.5) / 65536.0)
    e = LA.parse_chain([{"kind": "pitch_shift", "cents": [max(float(lo), -400.0), min(float(hi), 400.0)]}])[0]
    assert LA.speed_range(e) == (m, m)
    return e


def drawn(LA, chain, seed, step):
    """The speed offset the chain's pitch shift draws for this clip at this step; 0 where it does not fire."""
    chain = LA.parse_chain(chain)
    j = [a["kind"] for a in chain].index("pitch_shift")
    r = LA.entry_draw(seed, step, j)
    return LA.speed_offset(r[3], *LA.speed_range(chain[j])) if LA.fires(r[0], chain[j]["prob"]) else 0


# ---- 1. the operator alone ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def alone():
    """Two odd-length clips, shared by the tests of the stand-alone entry."""
    rng = np.random.default_rng(17)
    lengths = [4099, 7937]
    xs = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    return lengths, xs


@pytest.mark.parametrize("m", [M_MIN, M_MAX, -1, 0, 1, M_MID])
def test_pitch_shift_ola_against_the_restatement(rt, LA, alone, m):
    """aware_pitch_shift_ola, forward and adjoint, against the float64 restatement (autograd for the adjoint) on the f32
    operands; the samples at the clip's start, across the 1024-sample tile boundaries and at the clip's end are part of the
    whole-clip comparison and checked once more by index; the dot-product identity between the two directions.  The second clip
    starts at float offset 4099.  m = 0 is the identity, bit for bit, in both directions."""
    lengths, xs = alone
    rng = np.random.default_rng(m % 1000)
    gs = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    x = rt.Ragged.from_list(xs)
    z = rt.pitch_shift_ola(x, m)
    assert z.lengths == lengths and x.offsets[1] % 4 == 3
    gx = rt.pitch_shift_ola(rt.Ragged.from_list(gs), [m, m], adjoint=True)
    assert gx.lengths == lengths
    worst_f = worst_a = 0.0
    for xi, gi, zi, gxi, n in zip(xs, gs, z.to_list(), gx.to_list(), lengths):
        xt = torch.from_numpy(xi).double().requires_grad_(True)
        ref = LA.pitch_shift(xt, m)
        if m == 0:
            ref, refg = xi.astype(np.float64), gi.astype(np.float64)                   # the restatement returns x itself
        else:
            (ref * torch.from_numpy(gi).double()).sum().backward()
            ref, refg = ref.detach().numpy(), xt.grad.numpy()
        assert zi.shape == (n,) and gxi.shape == (n,)
        worst_f = max(worst_f, np.abs(zi - ref).max() / np.abs(ref).max())
        worst_a = max(worst_a, np.abs(gxi - refg).max() / np.abs(refg).max())
        for i in sorted(i for i in {0, 1, 255, 256, 1023, 1024, 1025, 4095, 4096, n - 2, n - 1}):
            assert abs(zi[i] - ref[i]) <= PITCH_BOUND * np.abs(ref).max(), (i, zi[i], ref[i])
            assert abs(gxi[i] - refg[i]) <= PITCH_BOUND * np.abs(refg).max(), (i, gxi[i], refg[i])
        if m == 0:
            assert np.array_equal(zi.view(np.uint32), xi.view(np.uint32))              # the identity, bit for bit
            assert np.array_equal(gxi.view(np.uint32), gi.view(np.uint32))
        a, b = float(np.dot(zi.astype(np.float64), gi)), float(np.dot(xi.astype(np.float64), gxi))
        # each side's error vector is at most PITCH_BOUND * peak per sample, and a peak is at most sqrt(n) times the rms
        slack = PITCH_BOUND * np.sqrt(n) * (np.linalg.norm(ref) * np.linalg.norm(gi) + np.linalg.norm(xi) * np.linalg.norm(refg))
        assert abs(a - b) <= slack, (a, b, slack)
    print(f"pitch_shift_ola m = {m}: max error / peak forward {worst_f:.2e}, adjoint {worst_a:.2e}")
    assert worst_f < PITCH_BOUND <= CAP and worst_a < PITCH_BOUND, (worst_f, worst_a)


def test_pitch_shift_ola_per_clip_offsets_and_errors(rt, LA, alone):
    lengths, xs = alone
    x = rt.Ragged.from_list(xs)
    # one offset per clip; a clip alone gives the same bits as inside a batch, wherever it starts
    z = rt.pitch_shift_ola(x, [M_MID, -777]).to_list()
    for xi, zi, m in zip(xs, z, (M_MID, -777)):
        np.testing.assert_array_equal(rt.pitch_shift_ola(rt.Ragged.from_list([xi]), [m]).to_list()[0], zi)
    # other output lengths than the clip's own: the first samples are the same bits, a longer output ends in zeros
    short = rt.pitch_shift_ola(x, M_MID, out_lengths=[3000, 9000]).to_list()
    np.testing.assert_array_equal(short[0], rt.pitch_shift_ola(x, M_MID).to_list()[0][:3000])
    np.testing.assert_array_equal(short[1][:7937], rt.pitch_shift_ola(x, M_MID).to_list()[1])
    assert np.all(short[1][7937 + 2:] == 0.0)
    from aware_amd import attacks as A
    atk = A.OverlapAddPitchShift(cents=-100.0)
    out = atk.apply_batch(x, 16000)
    assert out.lengths == lengths                                              # the output is as long as the input
    np.testing.assert_array_equal(out.to_list()[1], rt.pitch_shift_ola(x, atk.m).to_list()[1])
    np.testing.assert_array_equal(atk.apply(xs[0], 16000), out.to_list()[0])
    for bad in ([1], [0, M_MAX + 1], [M_MIN - 1, 0]):
        with pytest.raises(ValueError):
            rt.pitch_shift_ola(x, bad)
    with pytest.raises(ValueError):
        rt.pitch_shift_ola(x, 0, out_lengths=[4099])
    with pytest.raises(ValueError):
        rt.pitch_shift_ola(x, 0, out_lengths=[4099, 0])
    # the C entry copies a clip whose offset lies outside the range (the spans of the kernel are sized for the range)
    from aware_amd._lib import load_library
    md = torch.tensor([M_MAX + 1, M_MIN - 1], dtype=torch.int32, device="cuda")
    out = rt.Ragged(torch.empty(sum(lengths), dtype=torch.float32, device="cuda"), lengths)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert load_library().aware_pitch_shift_ola(p(x.data), p(x.d_off), p(x.d_len), p(out.data), p(out.d_off), p(out.d_len), 2,
                                                7937, p(md), 0, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.data, x.data)


# ---- 2. forward inside the loop -----------------------------------------------------------------------------------------------
def check_forward(LA, sess, batch, chain, seeds, step, tag, sample=None):
    torch.cuda.synchronize()
    worst = 0.0
    for b, y, z in sampled(sess, batch, sample):
        ref = LA.apply_chain(norm2(y.double())[None], chain, [seeds[b]], step)[0]
        worst = max(worst, float((z.double() - ref).abs().max() / ref.abs().max()))
    print(f"{tag}, step {step}: max |z - restatement| / peak = {worst:.2e}")
    assert worst < CHAIN_BOUND, (tag, step, worst)
    return worst


@pytest.mark.parametrize("name", list(CHAINS))
@pytest.mark.parametrize("lengths", [SHORT, LONG, RAGGED], ids=["short", "long", "ragged"])
def test_forward_matches_the_restatement(rt, O, LA, lengths, name):
    """Buffer 12 (sess.attacked) against apply_chain(N(N(buffer 9))) at steps 0, 2 and 17, within the project's bound for the
    loop's attacked signal (1.13e-6 of the peak).  Measured: 1.96e-7 at most over the 54 comparisons."""
    chain = LA.parse_chain(CHAINS[name])
    batch, seeds = forward_at_steps_0_2_17(rt, O, LA, chain, lengths, name, check_forward)
    assert len({drawn(LA, chain, seeds[0], s) for s in (0, 2, 17)}) == 3


@pytest.mark.parametrize("m", [M_MIN, M_MID, M_MAX])
@pytest.mark.parametrize("lengths", [LONG, RAGGED], ids=["long", "ragged"])
def test_step_0_is_the_stand_alone_entry(rt, O, LA, lengths, m):
    """With a range that holds one offset, buffer 12 at step 0 is aware_pitch_shift_ola on the same input, bit for bit: the
    loop's kernel and the stand-alone one share their arithmetic, whatever the partition into tiles.  The input x = N(N(y)) in
    the device's own rounding is buffer 12 of a second session whose entry never fires."""
    step_0_is_the_stand_alone_entry(rt, O, lengths, one_value(LA, m), lambda x: rt.pitch_shift_ola(x, m))


# ---- 3. first gradient ----------------------------------------------------------------------------------------------------------
# First clip seed of the gradient cases, chosen on the CPU so that the float64 restatement keeps every LeakyReLU argument of both
# clips at least 8e-6 from its kink: seeds 85 and 86: 4.4e-5 / 9.0e-5 (of the seeds 80 to 99 tried, 83 as the long clip was at
# 4.9e-8, 88 at 2.3e-7, 81 at 2.6e-6).  The case between two other entries, on two long clips: seeds 90 and 91: 3.5e-5 / 1.6e-5.
assert KINK == 8e-6
SEED0 = 85
SEED0_BETWEEN = 90


def check_first_gradient(rt, O, LA, chain, lengths, clip_seed0, **kw):
    """The figures of loop_support.first_gradient, with the bounds of the two sibling kinds: relative L2 of the gradient at most
    2e-5 for every clip, loss and prediction within 1e-6, and no clip closer than KINK to a LeakyReLU kink."""
    _, seeds, figures = first_gradient(rt, O, LA, chain, lengths, list(range(clip_seed0, clip_seed0 + len(lengths))), **kw)
    for i, (rel, kink, lerr, perr) in enumerate(figures):
        m = drawn(LA, chain, seeds[i], 0)
        print(f"{kw} clip {i} (n = {lengths[i]}, m = {m}): loss err {lerr:.1e}, pred err {perr:.1e}, "
              f"gradient rel L2 {rel:.2e}, nearest LeakyReLU kink {kink:.1e}")
        assert m != 0, "the case is to exercise the operator"
        assert kink >= KINK, (i, kink)
        assert lerr <= 1e-6 and perr <= 1e-6, (i, lerr, perr)
        assert rel <= 2e-5, (i, rel, kink)


@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
def test_first_gradient(rt, O, LA, dsp_path):
    """aware_embed_gradient against torch autograd over the restatement composed with the oracle's loop body, ragged batch:
    2e-5 relative L2 per clip, loss and prediction 1e-6.  Measured over the gradient tests of this file: 2.50e-6 relative L2 at
    most, loss 1.8e-7, prediction 3.9e-7; no clip closer than 1.6e-5 to a kink."""
    check_first_gradient(rt, O, LA, [PITCH], RAGGED, SEED0, dsp_path=dsp_path)


def test_first_gradient_f32_dense(rt, O, LA):
    check_first_gradient(rt, O, LA, [PITCH], RAGGED, SEED0, conv_pipe="f32", mel="dense")


def test_first_gradient_between_other_entries(rt, O, LA):
    """A suppression in front and noise behind: the stages on both sides of the fused adjoint."""
    check_first_gradient(rt, O, LA, [SUP, PITCH, NOISE10], LONG, SEED0_BETWEEN)


# ---- 4. graph replay, prob 0, workspace, error codes -------------------------------------------------------------------------------
def test_graph_replay_is_bit_identical_and_redraws(rt, O, LA):
    chain = [dict(PITCH, prob=0.75)]
    out, _ = graph_replay_bits(rt, O, chain, RAGGED)
    # the draw is keyed by the device step counter: clip 0 (seed 0) at steps 32..39 is shifted by the offsets the host draws
    ms = [drawn(LA, chain, 0, s) for s in range(32, 40)]
    assert len(set(ms)) >= 5, ms
    assert len({out[4][i].numpy().tobytes() for i in range(8)}) >= 5


def test_prob_0_is_the_plain_loop(rt, O):
    """A pitch shift that never fires, alone and between other entries that never fire either, against the loop without a
    chain: coefficients, best coefficients and losses after 20 steps and the gradient of step 20, bit for bit, on both
    dsp_paths (a clip on which no entry fires takes the plain loop's path)."""
    prob_0_is_the_plain_loop(rt, O, ([dict(PITCH, prob=0.0)], [dict(SUP, prob=0.0), dict(PITCH, prob=0.0), dict(NOISE10, prob=0.0)]))


def test_workspace_bytes(rt, O):
    """Chains of the older kinds need what they needed (the byte counts loop_support.PARENT_WORKSPACE holds); a chain with the new
    kind needs what the same chain with a speed change in its place needs."""
    size, nb, batch = older_chains_workspace(rt, O)
    assert size([ST]) == nb["speed"] and 4 * batch.total_out <= size([ST, SP]) - size([ST]) < 4 * batch.total_out + 256
    for with_ps, with_sp in (([PS], [SP]), ([NO, PS], [NO, SP]), ([NO, SU, PS, NO], [NO, SU, SP, NO]), ([PS, SU], [SP, SU])):
        assert size(with_ps) == size(with_sp) > nb["noise"]


def test_entry_point_error_codes(rt, O):
    from aware_amd._lib import LoopAttack
    sess, batch, _, _ = session(rt, O, RAGGED, [64, 65], None, num_iterations=20, use_graph=False)
    lib = sess.lib
    nb = lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries([PS]), 1)
    nb_rv = lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries([RV]), 1)
    big = max(nb, nb_rv) + 8 * batch.total_out + 512
    ws = torch.empty(big, dtype=torch.uint8, device="cuda")
    seeds = (C.c_uint32 * 2)(1, 2)

    def call(entries, n=None, wsb=big, sd=seeds):
        return lib.aware_embed_set_loop_attacks_ex(sess.h, ex_entries(entries), len(entries) if n is None else n, sd,
                                                   C.c_void_p(ws.data_ptr()), wsb, None)

    old = (LoopAttack * 1)(LoopAttack(5, 0.0, 1.0))
    assert lib.aware_embed_set_loop_attacks(sess.h, old, 1, seeds, C.c_void_p(ws.data_ptr()), big, None) == -1     # the older call
    assert call([(5, 1.0, [0.5, 3896.0])]) == -1 and call([(5, 1.0, [-3678.0, 3895.5])]) == -1      # not integers
    assert call([(5, 1.0, [10.0, 0.0])]) == -1 and call([(5, 1.0, [1.0, 0.0])]) == -1               # m_lo > m_hi
    assert call([(5, 1.0, [float(M_MIN - 1), 0.0])]) == -1 and call([(5, 1.0, [0.0, float(M_MAX + 1)])]) == -1
    assert call([(5, 1.0, [float("nan"), 0.0])]) == -1 and call([(5, 1.0, [0.0, float("inf")])]) == -1
    assert call([(5, 1.5, [0.0, 0.0])]) == -1
    assert call([PS, (5, 1.0, [0.0, 0.0])]) == -1 and call([PS, NO, PS]) == -1                      # a second pitch shift
    assert call([PS, RV]) == -1 and call([RV, PS]) == -1 and call([RV, NO, PS]) == -1               # beside a reverberation
    assert call([PS, SP]) == -1 and call([SP, PS]) == -1 and call([SP, NO, PS]) == -1 and call([PS, NO, SP]) == -1      # a speed change
    assert call([PS, ST]) == -1 and call([ST, PS]) == -1 and call([ST, NO, PS]) == -1 and call([PS, SU, ST]) == -1      # a time stretch
    assert call([ST, SP, PS]) == -1 and call([PS, ST, SP]) == -1
    assert call([PS], n=5) == -1 and call([PS], sd=None) == -1
    assert call([PS], wsb=nb - 256) == -4 and call([NO, PS], wsb=nb - 256) == -4
    assert call([(5, 1.0, [float(M_MIN), float(M_MAX)])], wsb=nb) == 0
    assert call([(5, 1.0, [0.0, 0.0])], wsb=nb) == 0
    assert call([PS], wsb=nb) == 0 and lib.aware_embed_buffer(sess.h, 12) and not lib.aware_embed_buffer(sess.h, 13)
    assert call([], n=0) == 0 and not lib.aware_embed_buffer(sess.h, 12)
    assert call([NO, SU, PS, NO], wsb=nb) == 0 and call([SU, PS], wsb=nb) == 0
    assert call([ST, SP]) == 0 and call([SP]) == 0 and call([RV]) == 0                             # the older chains still set
    assert call([PS], wsb=nb) == 0
    sess.iterate(1)
    torch.cuda.synchronize()
    assert call([PS]) == -1 and call([], n=0) == -1                        # after the first iterate
    with pytest.raises(ValueError):
        sess.set_loop_attacks([PITCH], [1, 2])


# ---- 5. the value claim on the device ---------------------------------------------------------------------------------------------
def test_value_claim_on_the_device(rt, O, tmp_path):
    """Four 1 s clips, seeds 0..3, 400 steps through AWAREEmbedder(loop_attacks=...) from an edited card, two embeddings: plain,
    and pitch_shift(+-150 cents, prob 0.75) in the loop.  Clean BER 0 % for both; under attacks.PitchShift (the phase vocoder,
    independent of the overlap-add operator) at -+50 and -+100 cents the plain BER is at least 25 % in the mean.
    attacks.TimeStretch at 0.9, 0.95, 1.05 and 1.1 is printed beside it.  The pitch-aware mean under the pitch shift is above
    two thirds of the plain mean on the CPU oracle (42.81 % against 51.88 %; tests/test_loop_pitch_host.py), so nothing is
    asserted about it here either: DESIGN.md section 19, "Limitation".  Measured on the MI355X, plain / pitch-aware BER in %:
    clean 0 / 0; pitch shift by -100 cents 61.25 / 41.25, -50 cents 46.25 / 43.75, +50 cents 50.00 / 47.50, +100 cents 47.50 /
    45.00, mean 51.25 / 44.38; phase vocoder stretch at 0.9 32.50 / 31.25, 0.95 38.75 / 27.50, 1.05 30.00 / 21.25, 1.1 38.75 /
    26.25, mean 35.00 / 26.56.  SNR against the normalised host, dB: plain 15.93, 15.12, 15.88, 16.08; pitch-aware 15.29, 15.53,
    16.15, 15.58."""
    from aware_amd import attacks as A
    from test_loop_pitch_host import AWARE_CHAIN, RATES, CENTS
    from test_loop_speed_host import snr_db
    clips, bits, embed, ber = value_claim_setup(O, tmp_path)

    ys = {}
    ys["plain"], det = embed(None)
    ys["pitch-aware"], _ = embed(AWARE_CHAIN)
    names = list(ys)
    clean = {k: ber(det, ys[k]) for k in names}
    print("clean BER: " + " / ".join(f"{k} {clean[k]:.2f} %" for k in names))
    ps = {k: [ber(det, A.PitchShift(cents=c).apply_batch(rt.Ragged.from_list(ys[k]), 16000)) for c in CENTS] for k in names}
    for i, c in enumerate(CENTS):
        print(f"pitch shift by {c:+d} cents: " + " / ".join(f"{k} {ps[k][i]:.2f} %" for k in names))
    st = {k: [ber(det, A.TimeStretch(rate=r).apply_batch(rt.Ragged.from_list(ys[k]), 16000)) for r in RATES] for k in names}
    for i, r in enumerate(RATES):
        print(f"phase vocoder stretch at {r}: " + " / ".join(f"{k} {st[k][i]:.2f} %" for k in names))
    mp = {k: float(np.mean(ps[k])) for k in names}
    ms = {k: float(np.mean(st[k])) for k in names}
    print("mean over the four pitch shifts: " + " / ".join(f"{k} {mp[k]:.2f} %" for k in names))
    print("mean over the four rates: " + " / ".join(f"{k} {ms[k]:.2f} %" for k in names))
    audio = np.stack(clips)
    for k in names:
        print(f"SNR against the normalised host, dB, {k}: " + ", ".join(f"{v:.2f}" for v in snr_db(np.stack(ys[k]), audio)))
    assert all(clean[k] == 0.0 for k in names)
    assert mp["plain"] >= 25.0
