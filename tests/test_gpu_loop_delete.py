"""Sample deletion inside the embed loop (EXTENSION, chain kind 7) on the device: the gather kernel of
csrc/loop_delete_kernels.hip and its adjoint twin, alone and inside the loop, against numpy slicing and the torch restatement
aware_amd/embedding/loop_attacks.py composed with the oracle's loop body.  Every value the operator writes is a copy, so the
comparisons are bit for bit wherever no noise entry follows.

Shapes: clips [8000] * 2 (7936 output samples), [16000] * 2 (15872, more than one synthesis run per clip) and the ragged
[16000, 8000]; stand-alone clips of 4099 and 7937 samples, packed back to back so that the second starts at an odd offset.

Run on the MI355X box:  python -m pytest tests/test_gpu_loop_delete.py -m gpu -q -s"""
import ctypes as C

import numpy as np
import pytest
import torch

from loop_support import CHAIN_BOUND, DS, KINK, LA, LONG, NO, NOISE10, O, PS, PV, RAGGED, RV, SHORT, SP, ST, SU, SUP, attacked
from loop_support import bits_equal, check_gradient, device_x, does_not_fire_keeps_its_bits, ex_entries, forward_at_steps_0_2_17
from loop_support import graph_replay_bits, norm2, older_chains_workspace, plus_zero, prob_0_is_the_plain_loop, rt, sampled
from loop_support import session, stereo_round_trip, synthesis, value_claim_setup

pytestmark = pytest.mark.gpu

CROP = {"kind": "delete_samples", "seconds": 0.032}
ANY = {"kind": "delete_samples", "seconds": [0.01, 0.2], "at": "anywhere"}
CHAINS = {"crop": [CROP], "anywhere": [ANY], "suppression_anywhere_noise": [SUP, ANY, NOISE10]}
assert CHAIN_BOUND == 1.13e-6                              # the project's bound for the loop's attacked signal


def cut(x, start, k):
    return np.concatenate([x[:start], x[start + k:], np.zeros(k, dtype=x.dtype)])


def cut_adjoint(g, start, k):
    return np.concatenate([g[:start], np.zeros(k, dtype=g.dtype), g[start:len(g) - k]])


def drawn(LA, chain, seed, step, ny):
    """(fires, start, k) of the chain's deletion for this clip at this step."""
    chain = LA.parse_chain(chain)
    j = [a["kind"] for a in chain].index("delete_samples")
    r = LA.entry_draw(seed, step, j)
    start, k = LA.delete_draw(chain[j], r, ny, 16000)
    return LA.fires(r[0], chain[j]["prob"]), start, k


# ---- 1. the operator alone ----------------------------------------------------------------------------------------------------
def test_delete_samples_is_numpy_bit_for_bit(rt):
    """aware_delete_samples, forward and adjoint, against slice-and-concatenate on uint32 views: a cut of one sample, one that
    crosses a workgroup's chunk, odd start and odd length, a cut that ends the clip, all but one sample, and k = 0; different
    values per clip in one call; exact zeros in the tail.  The second clip starts at float offset 4099."""
    rng = np.random.default_rng(17)
    lengths = [4099, 7937]
    xs = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    gs = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    x, g = rt.Ragged.from_list(xs), rt.Ragged.from_list(gs)
    assert x.offsets[1] % 4 == 3
    cases = [([0, 0], [1, 1]), ([0, 0], [513, 513]), ([1001, 3333], [777, 2049]), ([4099 - 300, 7937 - 4097], [300, 4097]),
             ([0, 0], [4098, 7936]), ([123, 7936], [0, 0]), ([0, 2047], [513, 1]), ([4098, 0], [1, 0])]
    for starts, ks in cases:
        z = rt.delete_samples(x, starts, ks).to_list()
        gx = rt.delete_samples(g, starts, ks, adjoint=True).to_list()
        for xi, gi, zi, gxi, s, k in zip(xs, gs, z, gx, starts, ks):
            assert bits_equal(zi, cut(xi, s, k)), (starts, ks)
            assert bits_equal(gxi, cut_adjoint(gi, s, k)), (starts, ks)
            assert np.all(zi[len(xi) - k:].view(np.uint32) == 0) and np.all(gxi[s:s + k].view(np.uint32) == 0)      # +0.0
            if k == 0:
                assert bits_equal(zi, xi) and bits_equal(gxi, gi)
    # one value for all clips; a clip alone gives the same bits as inside a batch, wherever it starts
    both = rt.delete_samples(x, 77, 513).to_list()
    for xi, zi in zip(xs, both):
        assert bits_equal(zi, cut(xi, 77, 513))
        assert bits_equal(rt.delete_samples(rt.Ragged.from_list([xi]), [77], [513]).to_list()[0], zi)
    for bad in (([0], [1]), ([0, 0], [4100, 1]), ([-1, 0], [1, 1]), ([4000, 0], [100, 1])):
        with pytest.raises(ValueError):
            rt.delete_samples(x, *bad)


# ---- 2. forward inside the loop -----------------------------------------------------------------------------------------------
def check_forward(LA, sess, batch, chain, seeds, step, tag, sample=None):
    torch.cuda.synchronize()
    exact = chain[-1]["kind"] != "gaussian_noise"
    worst = 0.0
    for b, y, z in sampled(sess, batch, sample):
        on, start, k = drawn(LA, chain, seeds[b], step, len(y))
        assert on and 1 <= k < len(y)
        if exact:
            ref = LA.apply_chain(torch.from_numpy(device_x(y.numpy()))[None], chain, [seeds[b]], step)[0]
            assert bits_equal(z.numpy(), ref.numpy()), (tag, step, b, start, k)
            assert np.all(z.numpy()[len(y) - k:].view(np.uint32) == 0)                     # the tail: exact zeros
        ref = LA.apply_chain(norm2(y.double())[None], chain, [seeds[b]], step)[0]
        worst = max(worst, float((z.double() - ref).abs().max() / ref.abs().max()))
    print(f"{tag}, step {step}: max |z - float64 restatement| / peak = {worst:.2e}" + (", bit-identical to the float32 one" if exact else ""))
    assert worst < CHAIN_BOUND, (tag, step, worst)


@pytest.mark.parametrize("name", list(CHAINS))
@pytest.mark.parametrize("lengths", [SHORT, LONG, RAGGED], ids=["short", "long", "ragged"])
def test_forward_matches_the_restatement(rt, O, LA, lengths, name):
    """Buffer 12 at steps 0, 2 and 17.  Deletion alone: bit-identical to the restatement on x = N(N(buffer 9)) in the device's
    rounding.  With noise behind it: within CHAIN_BOUND = 1.13e-6 of the peak of the float64 restatement (all chains are held
    to that as well).  The draws differ from step to step."""
    chain = LA.parse_chain(CHAINS[name])
    batch, seeds = forward_at_steps_0_2_17(rt, O, LA, chain, lengths, name, check_forward)
    assert len({drawn(LA, chain, seeds[0], s, batch.out_lengths[0])[1:] for s in (0, 2, 17)}) == 3


@pytest.mark.parametrize("name", ["crop", "anywhere", "suppression_anywhere"])
def test_step_0_is_the_restatement_on_the_device_own_input(rt, O, LA, name):
    """The input x = N(N(y)) in the device's own rounding is buffer 12 of a second session whose entries never fire; buffer 12 of
    the firing session at step 0 is the restatement on it, bit for bit, and so is the stand-alone entry."""
    chain = LA.parse_chain({"crop": [CROP], "anywhere": [ANY], "suppression_anywhere": [SUP, ANY]}[name])
    on, batch, _, _ = session(rt, O, RAGGED, [30, 31], chain, [3, 4])
    off, _, _, _ = session(rt, O, RAGGED, [30, 31], [dict(a, prob=0.0) for a in chain], [3, 4])
    on.gradient()
    off.gradient()
    torch.cuda.synchronize()
    assert torch.equal(on._view(9, (batch.total_out,)), off._view(9, (batch.total_out,)))
    xs = attacked(off, batch)
    for b, (x, y, z) in enumerate(zip(xs, synthesis(off, batch), attacked(on, batch))):
        assert bits_equal(x.numpy(), device_x(y.numpy()))
        ref = LA.apply_chain(x[None], chain, [3 + b], 0)[0].numpy()
        if name == "suppression_anywhere":
            assert not np.any(np.signbit(z.numpy()) & (z.numpy() == 0))                    # the device's zeros are +0.0
            ref = plus_zero(ref)
        assert bits_equal(z.numpy(), ref)
    if name != "suppression_anywhere":
        draws = [drawn(LA, chain, 3 + b, 0, n) for b, n in enumerate(batch.out_lengths)]
        alone = rt.delete_samples(rt.Ragged(off.attacked.clone(), batch.out_lengths), [d[1] for d in draws], [d[2] for d in draws])
        assert torch.equal(alone.data, on.attacked) and not torch.equal(alone.data, off.attacked)


# ---- 3. first gradient ----------------------------------------------------------------------------------------------------------
# Clip seeds chosen on the CPU so that both the float64 and the float32 restatement keep every LeakyReLU argument of both clips
# at least KINK = 8e-6 from its kink (seeds 80 to 95 tried).  Ragged [16000, 8000], the entry alone: seeds 82 and 83, 1.6e-5 /
# 6.3e-5 (80 as the long clip was at 7.2e-6, 81 at 5.7e-6).  Two long clips between a suppression and noise: seeds 94 and 95,
# 1.9e-5 / 1.3e-5 (80 as the first was at 5.3e-7, 84 as the second at 5.1e-7).
SEED0, SEED0_BETWEEN = 82, 94
assert KINK == 8e-6
# the module's pieces of loop_support.check_gradient, which states the rule and its bounds
GRADIENT = dict(drawn=drawn, describe=lambda d: f"start = {d[1]}, k = {d[2]}", exercised=lambda d, i, ny: d[0] and d[2] >= 1)


@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
def test_first_gradient(rt, O, LA, dsp_path):
    check_gradient(rt, O, LA, [ANY], RAGGED, SEED0, **GRADIENT, dsp_path=dsp_path)


def test_first_gradient_f32_dense(rt, O, LA):
    check_gradient(rt, O, LA, [ANY], RAGGED, SEED0, **GRADIENT, conv_pipe="f32", mel="dense")


@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
def test_first_gradient_between_other_entries(rt, O, LA, dsp_path):
    """A suppression in front and noise behind: the stages on both sides."""
    check_gradient(rt, O, LA, [SUP, ANY, NOISE10], LONG, SEED0_BETWEEN, **GRADIENT, dsp_path=dsp_path)


# ---- 4. per-clip and replay behaviour ---------------------------------------------------------------------------------------------
def test_a_clip_that_does_not_fire_keeps_its_bits(rt, O, LA):
    """prob 0.5 on three clips, 8 steps: where the entry does not fire, buffer 12 is N(N(buffer 9)) in the device's rounding,
    bit for bit; where it fires it is the cut of that.  Both occur."""
    does_not_fire_keeps_its_bits(rt, O, LA, ANY, drawn, apply=lambda x, z, d: bits_equal(z, cut(x, d[1], d[2])), fired=lambda d, ny: d[0])


def test_prob_0_is_the_plain_loop(rt, O):
    """A deletion that never fires against the loop without a chain: coefficients, best coefficients and losses after 20 steps
    and the gradient of step 20, bit for bit, alone and between two older entries that never fire either, on both dsp_paths."""
    prob_0_is_the_plain_loop(rt, O, ([dict(ANY, prob=0.0)], [dict(SUP, prob=0.0), dict(CROP, prob=0.0), dict(NOISE10, prob=0.0)]))


@pytest.mark.parametrize("lengths", [LONG, RAGGED], ids=["long", "ragged"])
def test_graph_replay_is_bit_identical_and_redraws(rt, O, LA, lengths):
    chain = LA.parse_chain([dict(ANY, prob=0.75), NOISE10])
    _, batch = graph_replay_bits(rt, O, chain, lengths)
    # the draws are keyed by the device step counter: both start and k of clip 0 (seed 0) move from step to step
    n0 = batch.out_lengths[0]
    draws = [drawn(LA, chain, 0, s, n0) for s in range(32, 40)]
    fired = [d for d in draws if d[0]]
    assert len({d[1] for d in fired}) >= 4 and len({d[2] for d in fired}) >= 4, draws
    # a second chain without the noise: the replayed graph's buffer 12 ends in exactly k zeros at every step
    bare = LA.parse_chain([ANY])
    sess, batch, _, _ = session(rt, O, lengths, list(range(50, 50 + len(lengths))), bare, num_iterations=40, use_graph=True)
    sess.iterate(4)
    ks = set()
    for step in range(4, 10):
        sess.iterate(1)
        torch.cuda.synchronize()
        z = attacked(sess, batch)[0].numpy()
        _, start, k = drawn(LA, bare, 0, step, n0)
        assert np.all(z[n0 - k:] == 0.0) and z[n0 - k - 1] != 0.0, (step, k)
        ks.add((start, k))
    assert len(ks) == 6


# ---- 5. workspace and error codes -------------------------------------------------------------------------------------------------
DSA = (7, 0.75, [160.0, 3200.0, 1.0])


def test_workspace_bytes(rt, O):
    """The seven older chains need what they needed; a chain with the kind needs what the same chain with a speed change in
    its place needs."""
    size, nb, _ = older_chains_workspace(rt, O)
    for with_ds, with_sp in (([DS], [SP]), ([DSA], [SP]), ([NO, DS], [NO, SP]), ([NO, SU, DSA, NO], [NO, SU, SP, NO]), ([DS, SU], [SP, SU])):
        assert size(with_ds) == size(with_sp) > nb["noise"]


def test_entry_point_error_codes(rt, O):
    from aware_amd._lib import LoopAttack
    sess, batch, _, _ = session(rt, O, RAGGED, [64, 65], None, num_iterations=20, use_graph=False)
    lib = sess.lib
    nb = lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries([DS]), 1)
    nb_rv = lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries([RV]), 1)
    nb_pv = lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries([PV]), 1)
    big = max(nb, nb_rv, nb_pv) + 8 * batch.total_out + 512
    ws = torch.empty(big, dtype=torch.uint8, device="cuda")
    seeds = (C.c_uint32 * 2)(1, 2)
    assert batch.out_lengths == [15872, 7936]

    def call(entries, n=None, wsb=big, sd=seeds):
        return lib.aware_embed_set_loop_attacks_ex(sess.h, ex_entries(entries), len(entries) if n is None else n, sd,
                                                   C.c_void_p(ws.data_ptr()), wsb, None)

    old = (LoopAttack * 1)(LoopAttack(7, 512.0, 1.0))
    assert lib.aware_embed_set_loop_attacks(sess.h, old, 1, seeds, C.c_void_p(ws.data_ptr()), big, None) == -1     # the older call
    assert call([(7, 1.0, [1.5, 512.0, 0.0])]) == -1 and call([(7, 1.0, [1.0, 511.5, 0.0])]) == -1                  # not integers
    assert call([(7, 1.0, [0.0, 512.0, 0.0])]) == -1 and call([(7, 1.0, [-3.0, 512.0, 0.0])]) == -1                 # k_lo < 1
    assert call([(7, 1.0, [513.0, 512.0, 0.0])]) == -1                                                              # k_lo > k_hi
    assert call([(7, 1.0, [1.0, 512.0, 2.0])]) == -1 and call([(7, 1.0, [1.0, 512.0, 0.5])]) == -1                  # other at values
    assert call([(7, 1.0, [1.0, 512.0, -1.0])]) == -1
    assert call([(7, 1.0, [float("nan"), 512.0, 0.0])]) == -1 and call([(7, 1.0, [1.0, float("inf"), 0.0])]) == -1
    assert call([(7, 1.0, [1.0, 512.0, float("nan")])]) == -1
    assert call([(7, 1.5, [1.0, 512.0, 0.0])]) == -1
    assert call([DS, DSA]) == -1 and call([DS, NO, DS]) == -1                                                       # a second entry
    for other in (RV, SP, ST, PS, PV):                                                                              # forbidden neighbours
        assert call([DS, other]) == -1 and call([other, DS]) == -1, other
        assert call([other, NO, DSA]) == -1 and call([DSA, SU, other]) == -1, other
    assert call([ST, SP, DS]) == -1 and call([DS, ST, SP]) == -1
    assert call([DS], n=5) == -1 and call([DS], sd=None) == -1
    assert call([DS], wsb=nb - 256) == -4 and call([NO, DSA], wsb=nb - 256) == -4                                   # too small
    assert call([(7, 1.0, [1.0, 7936.0, 0.0])]) == -2 and call([(7, 1.0, [7936.0, 7936.0, 1.0])]) == -2             # k_hi >= Ny
    assert call([SU, (7, 1.0, [1.0, 100000.0, 1.0])]) == -2
    assert call([(1, 1.0, [7936.0])]) == -2                                                                         # the suppression's code
    assert call([(7, 1.0, [1.0, 7935.0, 1.0])], wsb=nb) == 0
    assert call([DS], wsb=nb) == 0 and lib.aware_embed_buffer(sess.h, 12) and not lib.aware_embed_buffer(sess.h, 13)
    assert call([], n=0) == 0 and not lib.aware_embed_buffer(sess.h, 12)
    assert call([NO, SU, DSA, NO], wsb=nb) == 0 and call([SU, DS], wsb=nb) == 0
    assert call([ST, SP]) == 0 and call([SP]) == 0 and call([RV]) == 0 and call([PS]) == 0 and call([PV]) == 0      # the older chains still set
    assert call([DSA], wsb=nb) == 0
    sess.iterate(1)
    torch.cuda.synchronize()
    assert call([DS]) == -1 and call([], n=0) == -1                        # after the first iterate
    with pytest.raises(ValueError):
        sess.set_loop_attacks([CROP], [1, 2])
    # the host refuses a cut that is too long before any launch
    fresh, _, _, _ = session(rt, O, RAGGED, [64, 65], None, num_iterations=20, use_graph=False)
    with pytest.raises(ValueError, match="clip 1"):
        fresh.set_loop_attacks([{"kind": "delete_samples", "seconds": 0.5}], [1, 2])


# ---- 6. card round trip -----------------------------------------------------------------------------------------------------------
def test_stereo_service_round_trip_with_the_card_key(rt, tmp_path):
    """load() of a card with the deletion in loop_attacks, then embed_watermark / detect_watermark on a stereo clip: every
    channel carries the payload."""
    stereo_round_trip(tmp_path, "[{kind: delete_samples, seconds: 0.032, at: start, prob: 0.75}]", dict(CROP, prob=0.75))


# ---- 7. the value claim on the device ---------------------------------------------------------------------------------------------
def test_value_claim_on_the_device(rt, O, tmp_path):
    """The host test's two embeddings (four 1 s clips, seeds 0..3, 400 steps) through AWAREEmbedder(loop_attacks=...) from an
    edited card, evaluated by plain slicing at the host test's points with its bounds: clean 0 % both, the plain means over the
    crops and over the deletions at least 10 % each, the aware means at most half of them.  Figures: DESIGN.md section 21."""
    from test_loop_delete_host import AWARE_CHAIN, CROPS, DELETIONS
    from test_loop_speed_host import snr_db
    clips, bits, embed, ber = value_claim_setup(O, tmp_path)

    def table(det, y):
        return ([ber(det, y[:, d:]) for d in CROPS],
                [ber(det, np.concatenate([y[:, :s], y[:, s + k:]], axis=1)) for k, s in DELETIONS])

    y0, det = embed(None)
    y1, _ = embed(AWARE_CHAIN)
    y0, y1 = np.stack(y0), np.stack(y1)
    clean0, clean1 = ber(det, y0), ber(det, y1)
    print(f"clean BER plain {clean0:.2f} % / deletion-aware {clean1:.2f} %")
    c0, d0 = table(det, y0)
    c1, d1 = table(det, y1)
    for d, b0, b1 in zip(CROPS, c0, c1):
        print(f"first {d} samples dropped: plain {b0:.2f} % / deletion-aware {b1:.2f} %")
    for (k, s), b0, b1 in zip(DELETIONS, d0, d1):
        print(f"{k} samples cut out at {s}: plain {b0:.2f} % / deletion-aware {b1:.2f} %")
    mc0, mc1, md0, md1 = float(np.mean(c0)), float(np.mean(c1)), float(np.mean(d0)), float(np.mean(d1))
    print(f"mean over the crops: plain {mc0:.2f} % / deletion-aware {mc1:.2f} %; over the deletions: plain {md0:.2f} % / "
          f"deletion-aware {md1:.2f} %")
    audio = np.stack(clips)
    print("SNR against the normalised host, dB: plain " + ", ".join(f"{v:.2f}" for v in snr_db(y0, audio))
          + " / deletion-aware " + ", ".join(f"{v:.2f}" for v in snr_db(y1, audio)))
    assert clean0 == 0.0 and clean1 == 0.0
    assert mc0 >= 10.0 and md0 >= 10.0
    assert mc1 <= 0.5 * mc0
    assert md1 <= 0.5 * md0
