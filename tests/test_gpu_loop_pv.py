"""The phase vocoder inside the embed loop (EXTENSION) on the device: the two kernels of csrc/loop_pv_kernels.hip alone on a
ragged spectrum, between the library's STFT and iSTFT (runtime.pv_stretch), and as chain kind 6 inside the loop, against the
float64 torch restatement aware_amd/embedding/loop_attacks.py composed with the oracle's loop body.

Bounds.  The kernels alone see the same float32 spectrum as the restatement, so their bound is a cap from the count of
roundings (four times the largest error measured on the MI355X once that is known).  Everything behind an STFT cannot be held that way: the
restatement's transform differs from the device's in the last bits, and the phase error of a bin lasts for the rest of the
clip.  There the floor is what two float32 evaluations leave: the distance of the float32 torch restatement from the float64
one on the same input, computed on the CPU inside the test (no device code is involved), and the device is held within four
times that floor.

Shapes: spectra of 17 and 32 frames back to back (the second at an odd row); stand-alone clips of 4099 and 7937 samples; loop
clips [8000] * 2 (7936 output samples), [16000] * 2 (15872, more than one synthesis run per clip) and the ragged [16000, 8000].

Run on the MI355X box:  python -m pytest tests/test_gpu_loop_pv.py -m gpu -q -s"""
import ctypes as C

import numpy as np
import pytest
import torch

from loop_support import CHAIN_BOUND, KINK, LA, LONG, NO, NOISE10, O, PS, PV, RAGGED, RV, SHORT, SP, ST, SU, SUP, attacked
from loop_support import check_gradient, ex_entries, forward_at_steps_0_2_17, graph_replay_bits, norm2, older_chains_workspace
from loop_support import prob_0_is_the_plain_loop, rt, sampled, session, stereo_round_trip, value_claim_setup

pytestmark = pytest.mark.gpu

Q_MIN, Q_MAX, Q_MID = -16384, 21845, 4464                  # the stretch's range of offsets, and one inside
PV_RATE = {"kind": "phase_vocoder", "rate": [0.85, 1.15]}
PV_CENTS = {"kind": "phase_vocoder", "cents": 150.0}
PV_BOTH = {"kind": "phase_vocoder", "rate": [0.85, 1.15], "cents": 150.0}
CHAINS = {"stretch": [PV_RATE], "pitch": [PV_CENTS], "both": [PV_BOTH], "suppression_both_noise": [SUP, PV_BOTH, NOISE10]}
assert CHAIN_BOUND == 1.13e-6                              # the project's bound for the loop's attacked signal

# The two kernels against the float64 restatement on the same f32 spectrum, as a fraction of the reference's peak.  Indices
# and weights are exact on both sides; the device rounds |c| and u(c) of every cell (a division, a square root and three
# products each) and, per output frame, the two complex products and the Newton step that advance P: at most about ten
# roundings of 2^-24 per frame that can add up along the clip's 32 frames, and a handful on top for the interpolation or the
# gradient's two taps.  CAP is that count, 32 * 10 * 2^-24 + 8 * 2^-24 = 1.96e-5; it only says that PV_BOUND is sane.
# PV_BOUND is four times the largest measured error over the cases of the test.  MEASURED is the figure of the kernel's source
# compiled for the host on these inputs, 3.42e-7 forward (mq = 4464) and 2.62e-7 backward (mq = -16384): the kernel spells out
# its fused multiply-adds and HIP rounds divisions and square roots correctly, so the device differs from it only where the
# compiler contracts one of the few remaining products.  The test prints the device's figures.
CAP = (32 * 10 + 8) * 2.0 ** -24
MEASURED = 3.42e-7
PV_BOUND = 4 * MEASURED


@pytest.fixture(scope="module")
def plan(rt):
    return rt.Plan()


def pv_index(LA, chain):
    return [a["kind"] for a in LA.parse_chain(chain)].index("phase_vocoder")


def drawn(LA, chain, seed, step):
    """(fires, mq, m) of the chain's phase vocoder for this clip at this step."""
    chain = LA.parse_chain(chain)
    j = pv_index(LA, chain)
    r = LA.entry_draw(seed, step, j)
    return (LA.fires(r[0], chain[j]["prob"]),) + LA.pv_draw(chain[j], r)


# ---- 1. the kernels alone -------------------------------------------------------------------------------------------------------
FRAMES = [0, 17, 49]                                       # T = 17 and 32; the second clip starts at an odd row


@pytest.fixture(scope="module")
def spectra():
    """A seeded f32 spectrum of 49 rows with a zero frame and zero cells in each clip, and a gradient beside it."""
    rng = np.random.default_rng(23)
    S = (rng.standard_normal((49, 520)) + 1j * rng.standard_normal((49, 520))).astype(np.complex64)
    G = (rng.standard_normal((49, 520)) + 1j * rng.standard_normal((49, 520))).astype(np.complex64)
    S[:, 0], S[:, 512] = S[:, 0].real, S[:, 512].real
    S[5] = 0
    S[17 + 20] = 0
    S[0, 9] = S[3, 5] = S[16, 11] = S[17, 7] = S[48, 100] = 0
    return S, G


@pytest.mark.parametrize("mq", [Q_MIN, Q_MAX, -1, 0, 1, Q_MID])
def test_pv_frames_against_the_restatement(rt, LA, spectra, mq):
    """aware_pv_frames and aware_pv_frames_bwd against the float64 restatement (autograd for the backward) on the same f32
    spectrum, per clip, bins 0..512.  The pad columns come back zero.  mq = 0 returns its input bit for bit, both ways."""
    S, G = spectra
    Sd, Gd = torch.from_numpy(S).cuda(), torch.from_numpy(G).cuda()
    Y = rt.pv_frames(Sd, FRAMES, mq)
    gS = rt.pv_frames_bwd(Sd, Gd, FRAMES, [mq, mq])
    torch.cuda.synchronize()
    Y, gS = Y.cpu().numpy(), gS.cpu().numpy()
    assert np.all(Y[:, 513:] == 0) and np.all(gS[:, 513:] == 0)
    worst_f = worst_b = 0.0
    for a, b in zip(FRAMES, FRAMES[1:]):
        St = torch.from_numpy(S[a:b, :513].astype(np.complex128)).requires_grad_(True)
        ref = LA.pv_frames(St, mq)
        Gt = torch.from_numpy(G[a:b, :513].astype(np.complex128))
        if mq == 0:
            assert np.array_equal(Y[a:b, :513].view(np.uint32), S[a:b, :513].view(np.uint32))
            assert np.array_equal(gS[a:b, :513].view(np.uint32), G[a:b, :513].view(np.uint32))
            continue
        (ref.real * Gt.real + ref.imag * Gt.imag).sum().backward()
        ref, refg = ref.detach().numpy(), St.grad.numpy()
        worst_f = max(worst_f, np.abs(Y[a:b, :513] - ref).max() / np.abs(ref).max())
        worst_b = max(worst_b, np.abs(gS[a:b, :513] - refg).max() / np.abs(refg).max())
        assert np.all(gS[a:b, :513][S[a:b, :513] == 0] == 0)                          # d|c|/dc at a zero cell
        assert np.all(Y[a:b, :513][ref == 0] == 0)                                    # past the end of the clip: exact zeros
    print(f"pv_frames mq = {mq}: max error / peak forward {worst_f:.2e}, backward {worst_b:.2e}")
    assert worst_f < PV_BOUND <= CAP and worst_b < PV_BOUND, (worst_f, worst_b)


def test_pv_frames_in_place_per_clip_and_errors(rt, LA, spectra):
    S, G = spectra
    Sd, Gd = torch.from_numpy(S).cuda(), torch.from_numpy(G).cuda()
    # one offset per clip; a clip alone gives the same bits as inside the batch, wherever its rows start
    Y = rt.pv_frames(Sd, FRAMES, [Q_MID, -777])
    np.testing.assert_array_equal(rt.pv_frames(Sd[17:].contiguous(), [0, 32], [-777]).cpu().numpy(), Y[17:].cpu().numpy())
    np.testing.assert_array_equal(rt.pv_frames(Sd, [0, 17], [Q_MID])[:17].cpu().numpy(), Y[:17].cpu().numpy())
    # the backward may write over the spectrum it reads (the loop does): the same bits as out of place
    from aware_amd._lib import load_library
    ref = rt.pv_frames_bwd(Sd, Gd, FRAMES, [Q_MID, Q_MAX])
    work = Sd.clone()
    p = lambda t: C.c_void_p(t.data_ptr())
    fo = torch.tensor(FRAMES, dtype=torch.int32, device="cuda")
    md = torch.tensor([Q_MID, Q_MAX], dtype=torch.int32, device="cuda")
    assert load_library().aware_pv_frames_bwd(p(work), p(Gd), p(fo), 2, p(md), p(work), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(work[:, :513], ref[:, :513])
    # the C entry reads an offset outside the stretch's range as 0
    md = torch.tensor([Q_MAX + 1, Q_MIN - 1], dtype=torch.int32, device="cuda")
    out = torch.zeros_like(Sd)
    assert load_library().aware_pv_frames(p(Sd), p(fo), 2, p(md), p(out), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:, :513], Sd[:, :513])
    for bad in ([1], [0, Q_MAX + 1], [Q_MIN - 1, 0]):
        with pytest.raises(ValueError):
            rt.pv_frames(Sd, FRAMES, bad)
    with pytest.raises(ValueError):
        rt.pv_frames(Sd, [0, 17, 50], 5)
    with pytest.raises(ValueError):
        rt.pv_frames(Sd[:, :513], FRAMES, 5)


# ---- 2. between the transforms ----------------------------------------------------------------------------------------------------
def test_pv_stretch_against_the_restatement(rt, LA, plan):
    """runtime.pv_stretch on clips of 4099 and 7937 samples against the float64 restatement, at the range's ends and inside:
    within four times the distance of the float32 torch restatement from the float64 one on the same input, as a fraction of
    the reference's peak.  A clip with mq = 0 comes back as it is; every clip keeps its length."""
    rng = np.random.default_rng(17)
    lengths = [4099, 7937]
    xs = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    x = rt.Ragged.from_list(xs)
    for mqs in ([Q_MIN, Q_MAX], [Q_MAX, Q_MIN], [Q_MID, -Q_MID], [0, 3000]):
        z = rt.pv_stretch(plan, x, mqs)
        assert z.lengths == lengths
        for xi, zi, mq, n in zip(xs, z.to_list(), mqs, lengths):
            if mq == 0:
                assert np.array_equal(zi, xi)
                continue
            ref = LA.pv_stretch(torch.from_numpy(xi).double(), mq).numpy()
            r32 = LA.pv_stretch(torch.from_numpy(xi), mq).numpy()
            peak = np.abs(ref).max()
            floor, err = np.abs(r32 - ref).max() / peak, np.abs(zi - ref).max() / peak
            print(f"pv_stretch n = {n}, mq = {mq}: device {err:.2e} of the peak, float32 restatement {floor:.2e}")
            assert np.all(zi[256 * (n // 256):] == 0)
            assert err <= 4 * floor, (n, mq, err, floor)
    for bad in ([0, Q_MAX + 1], [Q_MIN - 1, 0], [1]):
        with pytest.raises(ValueError):
            rt.pv_stretch(plan, x, bad)


# ---- 3. forward inside the loop -----------------------------------------------------------------------------------------------
def check_forward(LA, sess, batch, chain, seeds, step, tag, sample=None):
    """Per clip: the device within four times the float32 restatement's distance from the float64 one, and never asked for
    more than the project's bound for the loop's attacked signal (the two normalisers' rounding alone reaches it)."""
    torch.cuda.synchronize()
    worst = worst_floor = 0.0
    by_floor = by_chain_bound = 0
    for b, y, z in sampled(sess, batch, sample):
        ref = LA.apply_chain(norm2(y.double())[None], chain, [seeds[b]], step)[0]
        r32 = LA.apply_chain(norm2(y.double()).float()[None], chain, [seeds[b]], step)[0]
        peak = float(ref.abs().max())
        floor, err = float((r32.double() - ref).abs().max()) / peak, float((z.double() - ref).abs().max()) / peak
        worst, worst_floor = max(worst, err), max(worst_floor, floor)
        assert err <= max(4 * floor, CHAIN_BOUND), (tag, step, b, err, floor, drawn(LA, chain, seeds[b], step))
        by_floor, by_chain_bound = by_floor + (4 * floor >= CHAIN_BOUND), by_chain_bound + (4 * floor < CHAIN_BOUND)
        print(f"{tag}, step {step}, clip {b} {drawn(LA, chain, seeds[b], step)}: |z - restatement| / peak = {err:.2e}, float32 restatement {floor:.2e}")
    print(f"{tag}, step {step}: max |z - restatement| / peak = {worst:.2e}, float32 restatement {worst_floor:.2e}; "
          f"{by_floor} clips held by four times the floor, {by_chain_bound} by the project's bound")


@pytest.mark.parametrize("name", list(CHAINS))
@pytest.mark.parametrize("lengths", [SHORT, LONG, RAGGED], ids=["short", "long", "ragged"])
def test_forward_matches_the_restatement(rt, O, LA, lengths, name):
    """Buffer 12 (sess.attacked) against apply_chain(N(N(buffer 9))) at steps 0, 2 and 17."""
    chain = LA.parse_chain(CHAINS[name])
    batch, seeds = forward_at_steps_0_2_17(rt, O, LA, chain, lengths, name, check_forward)
    assert len({drawn(LA, chain, seeds[0], s) for s in (0, 2, 17)}) == 3


def test_both_modes_occur_in_the_loop(LA):
    """The draws the forward test above sees with both keys hold both modes (host arithmetic only; no launch)."""
    modes = {drawn(LA, [PV_BOTH], 11 + 3 * i, s)[2] != 0 for i in range(2) for s in (0, 2, 17)}
    assert modes == {False, True}


# ---- 4. first gradient ----------------------------------------------------------------------------------------------------------
# Clip seeds chosen on the CPU so that both the float64 and the float32 restatement keep every LeakyReLU argument of both clips
# at least 8e-6 from its kink (seeds 80 to 99 tried).  Ragged [16000, 8000], the entry alone: seeds 83 and 84, 3.4e-5 / 3.2e-5
# (81 as the long clip was at 1.5e-6, 90 at 9.0e-7, 85 as the short one at 8.2e-7); both clips draw the stretch mode.  Two long
# clips between a suppression and noise: seeds 83 and 84, 2.9e-5 / 4.8e-5; the first draws the pitch mode, the second the
# stretch mode.
assert KINK == 8e-6
SEED0 = 83
SEED0_BETWEEN = 83


def gradient_case(modes):
    """The module's pieces of loop_support.check_gradient (the rule and its bounds are stated there):
    modes[i] says whether clip i is to draw the pitch mode."""
    return dict(drawn=lambda LA, chain, seed, step, ny: drawn(LA, chain, seed, step), describe=lambda d: f"mq = {d[1]}, m = {d[2]}",
                exercised=lambda d, i, ny: d[0] and d[1] != 0 and (d[2] != 0) == modes[i])


@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
def test_first_gradient(rt, O, LA, dsp_path):
    check_gradient(rt, O, LA, [PV_BOTH], RAGGED, SEED0, **gradient_case([False, False]), dsp_path=dsp_path)


def test_first_gradient_f32_dense(rt, O, LA):
    check_gradient(rt, O, LA, [PV_BOTH], RAGGED, SEED0, **gradient_case([False, False]), conv_pipe="f32", mel="dense")


@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
def test_first_gradient_between_other_entries(rt, O, LA, dsp_path):
    """A suppression in front and noise behind: the stages on both sides; the first clip is in pitch mode."""
    check_gradient(rt, O, LA, [SUP, PV_BOTH, NOISE10], LONG, SEED0_BETWEEN, **gradient_case([True, False]), dsp_path=dsp_path)


# ---- 5. invariants ----------------------------------------------------------------------------------------------------------------
def test_a_clip_that_does_not_fire_keeps_its_bits(rt, O, LA):
    """Noise in front of a vocoder that fires on one clip of two: the other clip's attacked signal and its gradient are those
    of the same chain with a vocoder that never fires, bit for bit (its u does not go through the transforms), while the firing
    clip differs.  Then the vocoder alone: the clip it leaves alone has z = N(N(y)), the plain loop's bits."""
    pv = dict(PV_BOTH, prob=0.5)
    seeds = next([a, a + 1] for a in range(0, 200, 2)
                 if drawn(LA, [NOISE10, pv], a, 0)[0] and drawn(LA, [NOISE10, pv], a, 0)[1] != 0 and not drawn(LA, [NOISE10, pv], a + 1, 0)[0])
    for chain in ([NOISE10, pv], [pv]):
        if len(chain) == 1:
            seeds = next([a, a + 1] for a in range(0, 200, 2)
                         if drawn(LA, chain, a, 0)[0] and drawn(LA, chain, a, 0)[1] != 0 and not drawn(LA, chain, a + 1, 0)[0])
        off_chain = [dict(a, prob=0.0) if a["kind"] == "phase_vocoder" else a for a in chain]
        on, batch, _, _ = session(rt, O, RAGGED, [30, 31], chain, seeds, use_graph=False)
        off, _, _, _ = session(rt, O, RAGGED, [30, 31], off_chain, seeds, use_graph=False)
        g_on, g_off = on.gradient(), off.gradient()
        torch.cuda.synchronize()
        z_on, z_off = attacked(on, batch), attacked(off, batch)
        assert torch.equal(z_on[1], z_off[1]) and not torch.equal(z_on[0], z_off[0])
        f = batch.frame_offsets
        assert torch.equal(g_on[f[1]:f[2]], g_off[f[1]:f[2]]) and not torch.equal(g_on[f[0]:f[1]], g_off[f[0]:f[1]])
        assert torch.equal(on.loss[1], off.loss[1])


def test_prob_0_is_the_plain_loop(rt, O):
    """A vocoder that never fires, alone and between two older entries that never fire either, against the loop without a chain:
    coefficients, best coefficients and losses after 20 steps and the gradient of step 20, bit for bit, on both dsp_paths."""
    prob_0_is_the_plain_loop(rt, O, ([dict(PV_BOTH, prob=0.0)], [dict(SUP, prob=0.0), dict(PV_BOTH, prob=0.0), dict(NOISE10, prob=0.0)]))


def test_graph_replay_is_bit_identical_and_redraws(rt, O, LA):
    chain = [dict(PV_BOTH, prob=0.75)]
    out, _ = graph_replay_bits(rt, O, chain, RAGGED)
    ds = [drawn(LA, chain, 0, s) for s in range(32, 40)]
    assert len(set(ds)) >= 5, ds
    assert len({out[4][i].numpy().tobytes() for i in range(8)}) >= 5


PVQ = (6, 0.75, [-9830.0, 9830.0, 0.0, -1.0])
PVM = (6, 0.75, [0.0, -1.0, -5435.0, 5930.0])


def test_workspace_bytes(rt, O):
    """The seven older chains need what they needed; a chain with the kind needs what the same chain with a speed change in its
    place needs and the two spectra of [total frames][520] complex values, each starting on a multiple of 256 bytes."""
    size, nb, batch = older_chains_workspace(rt, O)
    spec = batch.total_frames * 520 * 8
    spectra = (spec + 255) // 256 * 256 + spec
    print(f"workspace bytes: speed change {size([SP])}, phase vocoder {size([PV])}, two spectra {spectra}")
    assert size([SP]) % 256 == 0
    for with_pv, with_sp in (([PV], [SP]), ([PVQ], [SP]), ([PVM], [SP]), ([NO, PV], [NO, SP]), ([NO, SU, PV, NO], [NO, SU, SP, NO]),
                             ([PV, SU], [SP, SU])):
        assert size(with_pv) - size(with_sp) == spectra


def test_entry_point_error_codes(rt, O):
    from aware_amd._lib import LoopAttack
    sess, batch, _, _ = session(rt, O, RAGGED, [64, 65], None, num_iterations=20, use_graph=False)
    lib = sess.lib
    nb = lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries([PV]), 1)
    nb_rv = lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries([RV]), 1)
    big = max(nb, nb_rv) + 8 * batch.total_out + 512
    ws = torch.empty(big, dtype=torch.uint8, device="cuda")
    seeds = (C.c_uint32 * 2)(1, 2)

    def call(entries, n=None, wsb=big, sd=seeds):
        return lib.aware_embed_set_loop_attacks_ex(sess.h, ex_entries(entries), len(entries) if n is None else n, sd,
                                                   C.c_void_p(ws.data_ptr()), wsb, None)

    old = (LoopAttack * 1)(LoopAttack(6, 0.0, 1.0))
    assert lib.aware_embed_set_loop_attacks(sess.h, old, 1, seeds, C.c_void_p(ws.data_ptr()), big, None) == -1     # the older call
    assert call([(6, 1.0, [0.5, 9830.0, 0.0, -1.0])]) == -1 and call([(6, 1.0, [0.0, -1.0, -5435.0, 5929.5])]) == -1    # not integers
    assert call([(6, 1.0, [0.0, -1.0, 0.0, -1.0])]) == -1 and call([(6, 1.0, [5.0, 1.0, 9.0, 2.0])]) == -1              # no mode
    assert call([(6, 1.0, [float(Q_MIN - 1), 0.0, 0.0, -1.0])]) == -1 and call([(6, 1.0, [0.0, float(Q_MAX + 1), 0.0, -1.0])]) == -1
    assert call([(6, 1.0, [0.0, -1.0, -13521.0, 0.0])]) == -1 and call([(6, 1.0, [0.0, -1.0, 0.0, 17035.0])]) == -1
    assert call([(6, 1.0, [-100.0, 100.0, -13521.0, 0.0])]) == -1                                   # one good mode does not excuse the other
    assert call([(6, 1.0, [float("nan"), 0.0, 0.0, -1.0])]) == -1 and call([(6, 1.0, [0.0, -1.0, 0.0, float("inf")])]) == -1
    assert call([(6, 1.5, [0.0, 0.0, 0.0, -1.0])]) == -1
    assert call([PV, PVQ]) == -1 and call([PV, NO, PV]) == -1                                       # a second phase vocoder
    assert call([PV, RV]) == -1 and call([RV, PV]) == -1 and call([RV, NO, PV]) == -1               # beside a reverberation
    assert call([PV, SP]) == -1 and call([SP, PV]) == -1 and call([SP, NO, PV]) == -1 and call([PV, NO, SP]) == -1      # a speed change
    assert call([PV, ST]) == -1 and call([ST, PV]) == -1 and call([ST, NO, PV]) == -1 and call([PV, SU, ST]) == -1      # a time stretch
    assert call([PV, PS]) == -1 and call([PS, PV]) == -1 and call([PS, NO, PV]) == -1 and call([PV, SU, PS]) == -1      # a pitch shift
    assert call([ST, SP, PV]) == -1 and call([PV, ST, SP]) == -1
    assert call([PV], n=5) == -1 and call([PV], sd=None) == -1
    assert call([PV], wsb=nb - 256) == -4 and call([NO, PV], wsb=nb - 256) == -4
    assert call([(6, 1.0, [float(Q_MIN), float(Q_MAX), -13520.0, 17034.0])], wsb=nb) == 0
    assert call([PVQ], wsb=nb) == 0 and call([PVM], wsb=nb) == 0
    assert call([PV], wsb=nb) == 0 and lib.aware_embed_buffer(sess.h, 12) and not lib.aware_embed_buffer(sess.h, 13)
    assert call([], n=0) == 0 and not lib.aware_embed_buffer(sess.h, 12)
    assert call([NO, SU, PV, NO], wsb=nb) == 0 and call([SU, PV], wsb=nb) == 0
    assert call([ST, SP]) == 0 and call([SP]) == 0 and call([RV]) == 0 and call([PS]) == 0          # the older chains still set
    assert call([PV], wsb=nb) == 0
    sess.iterate(1)
    torch.cuda.synchronize()
    assert call([PV]) == -1 and call([], n=0) == -1                        # after the first iterate
    with pytest.raises(ValueError):
        sess.set_loop_attacks([PV_BOTH], [1, 2])


def test_stereo_service_round_trip_with_the_card_key(rt, tmp_path):
    """load() of a card with the phase vocoder in loop_attacks, then embed_watermark / detect_watermark on a stereo clip: every
    channel carries the payload."""
    stereo_round_trip(tmp_path, "[{kind: phase_vocoder, rate: [0.85, 1.15], cents: 150.0, prob: 0.9}]", dict(PV_BOTH, prob=0.9))


# ---- 6. the value claim on the device ---------------------------------------------------------------------------------------------
def test_value_claim_on_the_device(rt, O, tmp_path):
    """The host test's four embeddings (four 1 s clips, seeds 0..3, 400 steps) through AWAREEmbedder(loop_attacks=...) from an
    edited card, against attacks.PitchShift at -+50 and -+100 cents and attacks.TimeStretch at 0.9, 0.95, 1.05 and 1.1, with the
    host test's asserts: clean 0 %; plain means at least 25 % and 10 %; the stretch-aware stretch mean at most half the plain
    one; the pitch-aware pitch mean at most two thirds of the plain one; both keys meet both.  Figures: DESIGN.md section 20."""
    from aware_amd import attacks as A
    from test_loop_pv_host import CHAINS as VALUE_CHAINS, RATES, CENTS
    from test_loop_speed_host import snr_db
    clips, bits, embed, ber = value_claim_setup(O, tmp_path)

    ys = {}
    ys["plain"], det = embed(None)
    for k, chain in VALUE_CHAINS.items():
        ys[k], _ = embed(chain)
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
    assert mp["plain"] >= 25.0 and ms["plain"] >= 10.0
    assert ms["stretch-aware"] <= 0.5 * ms["plain"]
    assert mp["pitch-aware"] <= 2.0 / 3.0 * mp["plain"]
    assert ms["both"] <= 0.5 * ms["plain"] and mp["both"] <= 2.0 / 3.0 * mp["plain"]
