"""Sample deletion inside the embed loop (EXTENSION, chain kind 7) on the device: the gather kernel of
csrc/loop_delete_kernels.hip and its adjoint twin, alone and inside the loop, against numpy slicing and the torch restatement
aware_amd/embedding/loop_attacks.py composed with the oracle's loop body.  Every value the operator writes is a copy, so the
comparisons are bit for bit wherever no noise entry follows.

Shapes: clips [8000] * 2 (7936 output samples), [16000] * 2 (15872, more than one synthesis run per clip) and the ragged
[16000, 8000]; stand-alone clips of 4099 and 7937 samples, packed back to back so that the second starts at an odd offset.

Run on the MI355X box:  python -m pytest tests/test_gpu_loop_delete.py -m gpu -q -s"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, make_clip
from test_gpu_loop_attacks import attacked, norm2, sampled, session, synthesis
from test_gpu_loop_reverb import CHAIN_BOUND
from test_gpu_loop_stretch import PARENT_WORKSPACE, ex_entries
from test_gpu_loop_pv import KINK, oracle_gradient

pytestmark = pytest.mark.gpu

SHORT, LONG, RAGGED = [8000] * 2, [16000] * 2, [16000, 8000]
CROP = {"kind": "delete_samples", "seconds": 0.032}
ANY = {"kind": "delete_samples", "seconds": [0.01, 0.2], "at": "anywhere"}
NOISE10 = {"kind": "gaussian_noise", "snr_db": 10.0}
SUP = {"kind": "sample_suppression", "seconds": 0.3}
CHAINS = {"crop": [CROP], "anywhere": [ANY], "suppression_anywhere_noise": [SUP, ANY, NOISE10]}
assert CHAIN_BOUND == 1.13e-6                              # the project's bound for the loop's attacked signal


@pytest.fixture(scope="module")
def rt():
    from aware_amd import runtime
    from aware_amd._lib import require_gpu
    require_gpu()
    return runtime


@pytest.fixture(scope="module")
def O():
    from oracle import aware_oracle
    return aware_oracle


@pytest.fixture(scope="module")
def LA():
    from aware_amd.embedding import loop_attacks
    return loop_attacks


def cut(x, start, k):
    return np.concatenate([x[:start], x[start + k:], np.zeros(k, dtype=x.dtype)])


def cut_adjoint(g, start, k):
    return np.concatenate([g[:start], np.zeros(k, dtype=g.dtype), g[start:len(g) - k]])


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def plus_zero(a):
    """a with every -0.0 turned into +0.0 and every other bit kept (x + 0.0 in round-to-nearest).  The restatement suppresses by
    multiplying with a 0/1 mask, which leaves -0.0 under a negative sample; the device writes +0.0.  The sign of a suppressed
    zero is no part of the model."""
    return np.ascontiguousarray(a, dtype=np.float32) + np.float32(0.0)


def drawn(LA, chain, seed, step, ny):
    """(fires, start, k) of the chain's deletion for this clip at this step."""
    chain = LA.parse_chain(chain)
    j = [a["kind"] for a in chain].index("delete_samples")
    r = LA.entry_draw(seed, step, j)
    start, k = LA.delete_draw(chain[j], r, ny, 16000)
    return LA.fires(r[0], chain[j]["prob"]), start, k


def device_x(y):
    """x = N(N(y)) in the device's own rounding (csrc/common.hpp clip_norm_from_partials, chain_kernel): float32 throughout,
    m = max|y| + 1e-8, m2 = max|y| / m + 1e-8, x = (y * (1 / m)) * (1 / m2)."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    raw = np.float32(np.abs(y).max())
    m = np.float32(raw + np.float32(1e-8))
    m2 = np.float32(np.float32(raw / m) + np.float32(1e-8))
    return ((y * np.float32(np.float32(1.0) / m)) * np.float32(np.float32(1.0) / m2)).astype(np.float32)


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
    seeds = [11 + 3 * i for i in range(len(lengths))]
    sess, batch, _, _ = session(rt, O, lengths, list(range(20, 20 + len(lengths))), chain, seeds, num_iterations=20)
    assert sorted(batch.out_lengths)[0] in (7936, 15872)
    sess.gradient()
    check_forward(LA, sess, batch, chain, seeds, 0, name)
    sess.iterate(3)
    check_forward(LA, sess, batch, chain, seeds, 2, name)
    sess.iterate(15)
    assert int(sess.step.cpu()[0]) == 18
    check_forward(LA, sess, batch, chain, seeds, 17, name)
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


def check_gradient(rt, O, LA, chain, lengths, clip_seed0, **kw):
    """aware_embed_gradient against autograd over the float64 restatement composed with the oracle's loop body, with the rule
    and the bounds of test_gpu_loop_pv.py: relative L2 per clip within four times the float32 composition's own distance from
    the float64 one and at least 2e-5; loss and prediction the same way, at least 1e-6; no clip closer than KINK to a LeakyReLU
    kink in either precision."""
    clip_seeds = list(range(clip_seed0, clip_seed0 + len(lengths)))
    seeds = [5 + 2 * i for i in range(len(lengths))]
    sess, batch, pairs, wm = session(rt, O, lengths, clip_seeds, chain, seeds, use_graph=False, **kw)
    g = sess.gradient()
    torch.cuda.synchronize()
    g = g.cpu()
    loss, pred = sess.loss.cpu().numpy(), sess.pred.cpu().numpy()
    for i, (clip, _) in enumerate(pairs):
        ref, l, p, kink = oracle_gradient(O, LA, chain, seeds[i], clip, wm[i], torch.float64)
        r32, l32, p32, kink32 = oracle_gradient(O, LA, chain, seeds[i], clip, wm[i], torch.float32)
        floor = float((r32 - ref).norm() / ref.norm())
        lfloor, pfloor = abs(l32 - l), float(np.abs(p32 - p).max())
        mine = g[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :225].T.double()
        rel = float((mine - ref).norm() / ref.norm())
        lerr, perr = abs(loss[i] - l), float(np.abs(pred[i] - p).max())
        on, start, k = drawn(LA, chain, seeds[i], 0, batch.out_lengths[i])
        print(f"{kw} clip {i} (n = {lengths[i]}, start = {start}, k = {k}): loss err {lerr:.1e} (float32 restatement {lfloor:.1e}), pred err "
              f"{perr:.1e} ({pfloor:.1e}), gradient rel L2 {rel:.2e} ({floor:.2e}), nearest LeakyReLU kink {kink:.1e} / {kink32:.1e}")
        assert on and k >= 1, "the case is to exercise the operator"
        assert min(kink, kink32) >= KINK, (i, kink, kink32)
        assert lerr <= max(4 * lfloor, 1e-6) and perr <= max(4 * pfloor, 1e-6), (i, lerr, lfloor, perr, pfloor)
        assert rel <= max(4 * floor, 2e-5), (i, rel, floor)


@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
def test_first_gradient(rt, O, LA, dsp_path):
    check_gradient(rt, O, LA, [ANY], RAGGED, SEED0, dsp_path=dsp_path)


def test_first_gradient_f32_dense(rt, O, LA):
    check_gradient(rt, O, LA, [ANY], RAGGED, SEED0, conv_pipe="f32", mel="dense")


@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
def test_first_gradient_between_other_entries(rt, O, LA, dsp_path):
    """A suppression in front and noise behind: the stages on both sides."""
    check_gradient(rt, O, LA, [SUP, ANY, NOISE10], LONG, SEED0_BETWEEN, dsp_path=dsp_path)


# ---- 4. per-clip and replay behaviour ---------------------------------------------------------------------------------------------
def test_a_clip_that_does_not_fire_keeps_its_bits(rt, O, LA):
    """prob 0.5 on three clips, 8 steps: where the entry does not fire, buffer 12 is N(N(buffer 9)) in the device's rounding,
    bit for bit; where it fires it is the cut of that.  Both occur."""
    lengths, seeds = [16000, 8000, 24000], [1, 2, 3]
    chain = LA.parse_chain([dict(ANY, prob=0.5)])
    sess, batch, _, _ = session(rt, O, lengths, [70, 71, 72], chain, seeds, num_iterations=20)
    seen = set()
    for step in range(8):
        sess.iterate(1)
        torch.cuda.synchronize()
        for b, (y, z) in enumerate(zip(synthesis(sess, batch), attacked(sess, batch))):
            on, start, k = drawn(LA, chain, seeds[b], step, len(y))
            x = device_x(y.numpy())
            assert bits_equal(z.numpy(), cut(x, start, k) if on else x), (step, b, on)
            seen.add(on)
    assert seen == {False, True}


def test_prob_0_is_the_plain_loop(rt, O):
    """A deletion that never fires against the loop without a chain: coefficients, best coefficients and losses after 20 steps
    and the gradient of step 20, bit for bit, alone and between two older entries that never fire either, on both dsp_paths."""
    lengths = [8000, 16000, 24000]
    for dsp_path in ("stream", "staged"):
        plain, _, _, _ = session(rt, O, lengths, [62, 63, 64], None, num_iterations=21, dsp_path=dsp_path)
        plain.iterate(20)
        gp = plain.gradient()
        for chain in ([dict(ANY, prob=0.0)], [dict(SUP, prob=0.0), dict(CROP, prob=0.0), dict(NOISE10, prob=0.0)]):
            att, batch, _, _ = session(rt, O, lengths, [62, 63, 64], chain, num_iterations=21, dsp_path=dsp_path)
            att.iterate(20)
            ga = att.gradient()
            torch.cuda.synchronize()
            assert torch.equal(plain.coef, att.coef) and torch.equal(plain.best_coef, att.best_coef)
            assert torch.equal(plain.loss, att.loss) and torch.equal(plain.best_loss, att.best_loss)
            assert torch.equal(gp, ga)


@pytest.mark.parametrize("lengths", [LONG, RAGGED], ids=["long", "ragged"])
def test_graph_replay_is_bit_identical_and_redraws(rt, O, LA, lengths):
    chain = LA.parse_chain([dict(ANY, prob=0.75), NOISE10])
    out = []
    for use_graph in (True, False):
        sess, batch, _, _ = session(rt, O, lengths, list(range(50, 50 + len(lengths))), chain, num_iterations=40, use_graph=use_graph)
        zs, losses = [], []
        sess.iterate(32)
        for _ in range(8):
            sess.iterate(1)
            zs.append(sess.attacked.clone())
            losses.append(sess.loss.clone())
        torch.cuda.synchronize()
        out.append((sess.coef.cpu(), sess.best_coef.cpu(), sess.best_loss.cpu(), torch.stack(losses).cpu(), torch.stack(zs).cpu()))
        assert int(sess.step.cpu()[0]) == 40
    for a, b in zip(*out):
        assert torch.equal(a, b)
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
DS = (7, 0.75, [1.0, 512.0, 0.0])
DSA = (7, 0.75, [160.0, 3200.0, 1.0])
PV = (6, 0.9, [-9830.0, 9830.0, -5435.0, 5930.0])
PS = (5, 0.75, [-3678.0, 3896.0])
ST = (4, 0.75, [-9830.0, 9830.0])
SP = (3, 0.75, [-3678.0, 3896.0])
RV = (2, 1.0, [1600.0, 8000.0, -3.0])
NO = (0, 1.0, [10.0])
SU = (1, 1.0, [4800.0])


def test_workspace_bytes(rt, O):
    """The seven older chains need what they needed; a chain with the kind needs what the same chain with a speed change in
    its place needs."""
    sess, batch, _, _ = session(rt, O, RAGGED, [64, 65], None, num_iterations=20, use_graph=False)
    lib = sess.lib
    size = lambda ent: lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries(ent), len(ent))
    nb = {name: size(ent)
          for name, ent in (("noise", [NO]), ("noise_suppression", [NO, SU]), ("reverb", [RV]), ("suppression_reverb_noise", [SU, RV, NO]),
                            ("speed", [SP]), ("noise_speed", [NO, SP]), ("four", [NO, SU, SP, NO]))}
    assert nb == PARENT_WORKSPACE
    assert lib.aware_embed_loop_attack_workspace_bytes(batch.h, 2) == PARENT_WORKSPACE["noise_suppression"]
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
    from aware_amd.embedding.loop_attacks import parse_chain
    from aware_amd.service import detect_watermark, embed_watermark
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        card = yaml.safe_load(f)
    card["loop_attacks"] = yaml.safe_load("[{kind: delete_samples, seconds: 0.032, at: start, prob: 0.75}]")
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.loop_attacks == parse_chain([dict(CROP, prob=0.75)])
    bits = np.random.default_rng(29).integers(0, 2, 20).astype(np.int32)
    stereo = np.column_stack([make_clip(51, 16000)[0], make_clip(52, 16000)[0]])
    out = embed_watermark(stereo, 16000, bits, emb)
    assert out.shape[1] == 2 and np.isfinite(out).all()
    got = detect_watermark(out, 16000, det)
    for ch in (got if isinstance(got, (list, tuple)) else [got]):
        np.testing.assert_array_equal(np.asarray(ch).reshape(-1)[:20].astype(np.int32), bits)


# ---- 7. the value claim on the device ---------------------------------------------------------------------------------------------
def test_value_claim_on_the_device(rt, O, tmp_path):
    """The host test's two embeddings (four 1 s clips, seeds 0..3, 400 steps) through AWAREEmbedder(loop_attacks=...) from an
    edited card, evaluated by plain slicing at the host test's points with its bounds: clean 0 % both, the plain means over the
    crops and over the deletions at least 10 % each, the aware means at most half of them.  Figures: DESIGN.md section 21."""
    from aware_amd.utils.models import load
    from aware_amd.embedding.loop_attacks import parse_chain
    from test_loop_delete_host import AWARE_CHAIN, CROPS, DELETIONS
    from test_loop_speed_host import snr_db
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        card = yaml.safe_load(f)
    pairs = [make_clip(s, 16000) for s in range(4)]
    clips, bits = [p[0] for p in pairs], np.stack([p[1] for p in pairs])
    wm = np.stack([O.bits_to_bipolar(b) for b in bits]).astype(np.float32)

    def embed(chain):
        c = dict(card)
        if chain:
            c["loop_attacks"] = chain
        p = tmp_path / "card.yaml"
        p.write_text(yaml.safe_dump(c))
        emb, det = load(str(p))
        assert emb.loop_attacks == parse_chain(chain)
        return np.stack([o.cpu().numpy() for o in emb.embed_batch(clips, 16000, wm)]), det

    def ber(det, ys):
        vals = det.detect_batch(list(ys), 16000).cpu().numpy()
        return 100.0 * float((O.decode_bits(vals) != bits).mean())

    def table(det, y):
        return ([ber(det, y[:, d:]) for d in CROPS],
                [ber(det, np.concatenate([y[:, :s], y[:, s + k:]], axis=1)) for k, s in DELETIONS])

    y0, det = embed(None)
    y1, _ = embed(AWARE_CHAIN)
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
