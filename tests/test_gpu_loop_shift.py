"""Frequency shifts inside the embed loop (EXTENSION, chain kind 12) on the device: the kernel of csrc/loop_shift_kernels.hip alone
and inside the loop, against the float64 restatement aware_amd/embedding/loop_attacks.py (frequency_shift,
frequency_shift_adjoint) composed with the oracle's loop body.

Bounds.  Output: 128 f32 multiply-adds on taps within 1e-6 of the float64 ones, the sine and cosine of an argument that is exact
in f32, and the two products of the modulation: |z - ref| <= 2^-16 (1 + sum|h|) max|x| against the float64 restatement, the band
filter's own bound form with half its terms (sum|h| = 3.4103).  Adjoint: the two sides of <Ax, w> = <x, A^T w> differ by at most
that per output, so 2^-15 (1 + sum|h|) max|x| sum|w|.

Shapes: stand-alone clips of [100, 254, 255, 256, 4099, 8193, 16384] samples (two shorter than the taps, their count and one more,
one and two workgroup tiles crossed, four tiles exactly), packed back to back so that every clip but the first starts where its
neighbour ends, once with the whole buffer one float off its alignment; in the loop [16000, 8000] and [16000, 8000, 513] (the
shortest clip the loop takes) at a synthesis run of 4 hop blocks, and the batches that select runs of 12, 8 and 6.

Run on the MI355X box:  python -m pytest tests/test_gpu_loop_shift.py -m gpu -q -s"""
import ctypes as C

import numpy as np
import pytest
import torch

from loop_support import CHAIN_BOUND, DS, EV, FB, LA, NO, NOISE10, O, PS, PV, RAGGED, RV, SP, ST, SU, WC, XC
from loop_support import check_first_gradient, device_x, does_not_fire_keeps_its_bits, ex_entries, forward_at_run_length
from loop_support import forward_at_steps_0_2_17, graph_replay_bits, mixture_is_its_chains, norm2, older_chains_workspace
from loop_support import prob_0_is_the_plain_loop, rt, sampled, session, step_0_is_the_stand_alone_entry, stereo_round_trip
from loop_support import value_claim_setup
from test_loop_shift_host import ONE, PHASES, SHIFTS, SUM_H

pytestmark = pytest.mark.gpu

TINY = [16000, 8000, 513]
FSH = {"kind": "frequency_shift", "hz": 120.0}
ENV = {"kind": "gain_envelope", "period": [0.05, 0.5], "floor": 0.25}
SUP = {"kind": "sample_suppression", "seconds": 0.02}      # this module's own: short enough for the 513-sample clip of TINY
CHAINS = {"shift": [FSH], "noise_shift_envelope": [NOISE10, FSH, ENV], "suppression_shift": [SUP, FSH], "shift_noise": [FSH, NOISE10]}
FS = (12, 0.75, [-7864.0, 7864.0, 0.0, 0.0])               # the C ABI's entry of {hz: 120.0, prob: 0.75} at 16 kHz
TILE = 4096                                                 # outputs per workgroup of the stand-alone grid (kFsTile)
GAIN = 1.0 + SUM_H                                          # |x cos| + |Hx sin| <= (1 + sum|h|) max|x|
assert CHAIN_BOUND == 1.13e-6


def bound_of(xmax):
    return 2.0 ** -16 * GAIN * float(xmax)


def drawn(LA, chain, seed, step, ny=None):
    """(fires, d, p0) of the chain's frequency shift for this clip at this step."""
    chain = LA.parse_chain(chain)
    j = [a["kind"] for a in chain].index("frequency_shift")
    r = LA.entry_draw(seed, step, j)
    return (LA.fires(r[0], chain[j]["prob"]),) + LA.shift_draw(chain[j], r, 16000)


# ---- 1. the operator alone ----------------------------------------------------------------------------------------------------
LENGTHS = [100, 254, 255, 256, 4099, 8193, 16384]
COMBOS = [(d, p0) for d in SHIFTS for p0 in PHASES]


@pytest.fixture(scope="module")
def alone(LA):
    """The clips, the cotangents, and the float64 restatement in both directions for every (d, p0) a case uses, computed once."""
    rng = np.random.default_rng(29)
    xs = [rng.standard_normal(n).astype(np.float32) for n in LENGTHS]
    for x in xs:                                             # non-zero up to both ends: a halo that reads a neighbour shows
        x[0], x[-1] = 1.5, -1.5
    ws = [rng.standard_normal(n).astype(np.float32) for n in LENGTHS]
    refs = {}

    def ref(b, d, p0):
        if (b, d, p0) not in refs:
            refs[(b, d, p0)] = (LA.frequency_shift(torch.from_numpy(xs[b]).double(), d, p0).numpy(),
                                LA.frequency_shift_adjoint(torch.from_numpy(ws[b]).double(), d, p0).numpy())
        return refs[(b, d, p0)]

    return xs, ws, ref


def packed(rt, clips, lead):
    """The clips back to back in one device buffer that starts `lead` floats behind an aligned address."""
    flat = torch.from_numpy(np.concatenate(clips)).cuda()
    buf = torch.zeros(flat.numel() + lead + 8, dtype=torch.float32, device="cuda")
    buf[lead:lead + flat.numel()] = flat
    return rt.Ragged(buf[lead:lead + flat.numel()], [len(c) for c in clips])


@pytest.mark.parametrize("rot,lead", [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (2, 1)], ids=["r0", "r1", "r2", "r3", "r4", "r2_off_by_one_float"])
def test_output_and_adjoint(rt, alone, rot, lead):
    """Every (d, p0) of the host test on clips of every length, both directions, against the float64 restatement; once with the
    input and output buffers one float off their alignment: the unaligned store path."""
    xs, ws, ref = alone
    pick = [COMBOS[(2 * b + 3 * rot) % len(COMBOS)] for b in range(len(LENGTHS))]
    ds, ps = [p[0] for p in pick], [p[1] for p in pick]
    x, w = packed(rt, xs, lead), packed(rt, ws, lead)
    outz, outa = packed(rt, [np.zeros_like(v) for v in xs], lead), packed(rt, [np.zeros_like(v) for v in xs], lead)
    assert x.data.data_ptr() % 16 == 4 * lead and outz.data.data_ptr() % 16 == 4 * lead
    z = rt.frequency_shift(x, ds, ps, out=outz)
    aw = rt.frequency_shift(w, ds, ps, adjoint=True, out=outa)
    torch.cuda.synchronize()
    worst_z = worst_t = worst_a = 0.0
    for b, (xb, wb, zb, awb) in enumerate(zip(xs, ws, z.to_list(), aw.to_list())):
        rz, ra = ref(b, ds[b], ps[b])
        bz, bt = bound_of(np.abs(xb).max()), bound_of(np.abs(wb).max())
        zerr, terr = float(np.abs(zb.astype(np.float64) - rz).max()), float(np.abs(awb.astype(np.float64) - ra).max())
        worst_z, worst_t = max(worst_z, zerr / bz), max(worst_t, terr / bt)
        assert zerr <= bz, (b, LENGTHS[b], pick[b], zerr, bz)
        assert terr <= bt, (b, LENGTHS[b], pick[b], terr, bt)
        lhs, rhs = float(np.dot(zb.astype(np.float64), wb.astype(np.float64))), float(np.dot(xb.astype(np.float64), awb.astype(np.float64)))
        abound = 2.0 ** -15 * GAIN * float(np.abs(xb).max()) * float(np.abs(wb).sum())
        worst_a = max(worst_a, abs(lhs - rhs) / abound)
        assert abs(lhs - rhs) <= abound, (b, pick[b], lhs, rhs, abound)
    print(f"rot {rot}, lead {lead}: forward error / bound = {worst_z:.4f}; adjoint error / bound = {worst_t:.4f}; adjoint gap / bound = {worst_a:.5f}")


def test_alone_details(rt, alone):
    xs, ws, ref = alone
    x = rt.Ragged.from_list(xs)
    # one value for all clips; a clip alone gives the same bits as inside a batch, wherever it starts
    both = rt.frequency_shift(x, 3277, 5).to_list()
    for b in (0, 2, 4, 6):
        one = rt.frequency_shift(rt.Ragged.from_list([xs[b]]), [3277], [5]).to_list()[0]
        assert np.array_equal(one.view(np.uint32), both[b].view(np.uint32)), b
    # d = 0 at phase 0 is the identity, bit for bit: cos 1, sin 0
    same = rt.frequency_shift(x, 0, 0).to_list()
    assert all(np.array_equal(s.view(np.uint32), v.view(np.uint32)) for s, v in zip(same, xs))
    for bad in (([1], [0]), (65537, 0), (-65537, 0), (1, -1), (1, ONE)):
        with pytest.raises(ValueError):
            rt.frequency_shift(x, *bad)
    with pytest.raises(ValueError):
        rt.frequency_shift(x, 1, 0, out=x)
    from aware_amd import attacks as A
    got = A.FrequencyShift(50.0).apply_batch(x, 16000).to_list()
    want = rt.frequency_shift(x, 3277, 0).to_list()
    assert np.array_equal(got[4].view(np.uint32), want[4].view(np.uint32)) and A.FrequencyShift(-20.0, 0.5).apply(xs[4], 16000).shape == (4099,)
    with pytest.raises(ValueError):
        A.FrequencyShift(1200.0).apply_batch(x, 16000)


@pytest.mark.parametrize("adjoint", [False, True], ids=["forward", "adjoint"])
@pytest.mark.parametrize("n", [100, 255, 4099])
def test_nothing_is_written_past_the_clip(rt, LA, n, adjoint):
    """One clip written into the middle of a buffer of sentinels, at an address one float off its alignment: the sentinels on
    both sides keep their bits, and the clip is the operator's output."""
    rng = np.random.default_rng(n)
    xb = rng.standard_normal(n).astype(np.float32)
    big = torch.full((n + 64,), 7.25, dtype=torch.float32, device="cuda")
    out = rt.Ragged(big[33:33 + n], [n])
    rt.frequency_shift(rt.Ragged.from_list([xb]), [-7864], [ONE - 1], adjoint=adjoint, out=out)
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    assert np.all(got[:33] == 7.25) and np.all(got[33 + n:] == 7.25), n
    op = LA.frequency_shift_adjoint if adjoint else LA.frequency_shift
    ref = op(torch.from_numpy(xb).double(), -7864, ONE - 1).numpy()
    assert float(np.abs(got[33:33 + n] - ref).max()) <= bound_of(np.abs(xb).max())


# ---- 2. forward inside the loop -----------------------------------------------------------------------------------------------
def check_forward(LA, sess, batch, chain, seeds, step, tag, sample=None):
    """Against the float64 restatement on x = N(N(buffer 9)) in the device's rounding, to the stand-alone bound
    2^-16 (1 + sum|h|) max|x| of the shift's input.  With a noise entry the device's noise is f32 and within the project's
    CHAIN_BOUND of the peak of the float64 one: in front of the shift that passes through it, at most 1 + sum|h| times as large;
    behind it, it adds to the shift's own bound.  A gain envelope behind the shift multiplies both sides by gains of at most 1."""
    torch.cuda.synchronize()
    noisy = any(a["kind"] == "gaussian_noise" for a in chain)
    worst = 0.0
    for b, y, z in sampled(sess, batch, sample):
        on, d, p0 = drawn(LA, chain, seeds[b], step)
        assert on
        x = torch.from_numpy(device_x(y.numpy())).double() if not noisy else norm2(y.double())
        ref = LA.apply_chain(x[None], chain, [seeds[b]], step)[0]
        j = [a["kind"] for a in chain].index("frequency_shift")
        xin = LA.apply_chain(x[None], chain[:j], [seeds[b]], step)[0] if j else x
        bound = bound_of(xin.abs().max())
        if noisy:
            bound += CHAIN_BOUND * (GAIN * float(xin.abs().max()) + float(ref.abs().max()))
        err = float((z.double() - ref).abs().max())
        worst = max(worst, err / bound)
        assert err <= bound, (tag, step, b, (d, p0), err, bound)
    print(f"{tag}, step {step}: max |z - restatement| / bound = {worst:.4f}")


@pytest.mark.parametrize("name", list(CHAINS))
@pytest.mark.parametrize("lengths", [RAGGED, TINY], ids=["ragged", "tiny"])
def test_forward_matches_the_restatement(rt, O, LA, lengths, name):
    """Steps 0, 2 and 17 at a synthesis run of 4 hop blocks, alone and between noise and a gain envelope."""
    chain = LA.parse_chain(CHAINS[name])
    batch, seeds = forward_at_steps_0_2_17(rt, O, LA, chain, lengths, name, check_forward, shortest=(512, 7936))
    assert batch.synth_run == 4
    assert len({drawn(LA, chain, seeds[0], s)[1:] for s in (0, 2, 17)}) == 3


def test_step_0_is_the_stand_alone_entry(rt, O, LA):
    """Buffer 12 at step 0 is aware_frequency_shift with the host's draw on the same input, bit for bit: the loop's kernel and the
    stand-alone one share their arithmetic, and the kernel's draws are the host's."""
    def alone(x):
        d = [drawn(LA, [FSH], seed, 0) for seed in (3, 4)]
        assert all(v[0] for v in d)
        return rt.frequency_shift(x, [v[1] for v in d], [v[2] for v in d])

    step_0_is_the_stand_alone_entry(rt, O, RAGGED, FSH, alone)


@pytest.mark.parametrize("bname", ["R12", "R8", "R6"])
def test_forward_at_every_synthesis_run_length(rt, O, LA, bname):
    """The batches of tests/test_loop_run_rule_host.py that select synthesis runs of 12, 8 and 6 hop blocks (every other session of
    this module runs at 4, which test_forward_matches_the_restatement asserts): buffer 12 of the five head clips (18432, 16000,
    8000, 24000 and 513 samples) at steps 0 and 2 to the stand-alone bound.  A workgroup's share of a clip then spans up to 3072
    samples, and its halo reads its neighbours' shares."""
    forward_at_run_length(rt, O, LA, bname, "shift", LA.parse_chain([FSH]), check_forward)


# ---- 3. first gradient ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conv_pipe", ["bf16x3", "f16x2"])
def test_first_gradient(rt, O, LA, conv_pipe):
    """aware_embed_gradient with the chain against torch autograd over the restatement composed with the oracle's loop body, by
    loop_support.check_first_gradient: 2e-5 relative L2 per clip (2e-2 within 2e-6 of a LeakyReLU kink), loss and prediction
    1e-5."""
    check_first_gradient(rt, O, LA, [FSH], RAGGED, conv_pipe=conv_pipe)


@pytest.mark.parametrize("conv_pipe", ["bf16x3", "f16x2"])
def test_first_gradient_between_other_entries(rt, O, LA, conv_pipe):
    """Noise in front and a gain envelope behind: the stages on both sides of the shift's adjoint."""
    check_first_gradient(rt, O, LA, [NOISE10, FSH, ENV], RAGGED, conv_pipe=conv_pipe)


# ---- 4. per-clip and replay behaviour ---------------------------------------------------------------------------------------------
def test_a_clip_that_does_not_fire_keeps_its_bits(rt, O, LA):
    """prob 0.5 on three clips, 8 steps: where the entry does not fire, buffer 12 is N(N(buffer 9)) in the device's rounding, bit
    for bit; where it fires it is the drawn shift of that, to the stand-alone bound.  Both occur."""
    def shifted(x, z, d):
        ref = LA.frequency_shift(torch.from_numpy(x).double(), d[1], d[2]).numpy()
        return float(np.abs(z - ref).max()) <= bound_of(np.abs(x).max())

    does_not_fire_keeps_its_bits(rt, O, LA, FSH, drawn, apply=shifted, fired=lambda d, ny: d[0])


def test_prob_0_is_the_plain_loop(rt, O):
    """A shift that never fires against the loop without a chain: coefficients, best coefficients and losses after 20 steps and
    the gradient of step 20, bit for bit, alone and between two older entries that never fire either, on both dsp_paths."""
    prob_0_is_the_plain_loop(rt, O, ([dict(FSH, prob=0.0)], [dict(SUP, prob=0.0), dict(FSH, prob=0.0), dict(NOISE10, prob=0.0)]))


def test_graph_replay_is_bit_identical_and_redraws(rt, O, LA):
    chain = LA.parse_chain([dict(FSH, prob=0.75), NOISE10])
    out, _ = graph_replay_bits(rt, O, chain, RAGGED)
    # the draws are keyed by the device step counter: the replayed graph's buffer 12 moves with them
    zs = out[4]
    assert len({zs[i].numpy().tobytes() for i in range(8)}) == 8
    draws = [drawn(LA, chain, 0, s) for s in range(32, 40)]
    assert len({d[1:] for d in draws if d[0]}) >= 4, draws


def test_a_mixture_is_its_chains(rt, O, LA):
    """A mixture of a shift chain and a noise chain at step 0 against, per clip, a session that holds only the chain the clip
    drew: buffers 12 and 9, loss, prediction and the rows of the coefficient gradient, bit for bit."""
    mixture_is_its_chains(rt, O, LA, [FSH, NOISE10], [NOISE10])


# ---- 5. workspace and error codes -------------------------------------------------------------------------------------------------
def test_workspace_bytes(rt, O):
    """The seven older chains need what they needed (PARENT_WORKSPACE); a chain with the kind needs what the same chain with a
    deletion in its place needs."""
    size, nb, _ = older_chains_workspace(rt, O)
    for with_fs, with_ds in (([FS], [DS]), ([NO, FS], [NO, DS]), ([NO, SU, FS, NO], [NO, SU, DS, NO]), ([EV, FS, EV], [EV, DS, EV])):
        assert size(with_fs) == size(with_ds) > nb["noise"]
    for other in (RV, SP, ST, PS, PV, DS, FB, XC):          # a refused chain is sized by the older kind, as before
        assert size([FS, other]) == size([other, FS]) == size([other])


def test_entry_point_error_codes(rt, O):
    from aware_amd._lib import LoopAttack
    sess, batch, _, _ = session(rt, O, RAGGED, [64, 65], None, num_iterations=20, use_graph=False)
    lib = sess.lib
    nb = lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries([FS]), 1)
    big = max(nb, lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries([RV]), 1),
              lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries([PV]), 1)) + 8 * batch.total_out + 512
    ws = torch.empty(big, dtype=torch.uint8, device="cuda")
    seeds = (C.c_uint32 * 2)(1, 2)

    def call(entries, n=None, wsb=big, sd=seeds):
        return lib.aware_embed_set_loop_attacks_ex(sess.h, ex_entries(entries), len(entries) if n is None else n, sd,
                                                   C.c_void_p(ws.data_ptr()), wsb, None)

    old = (LoopAttack * 1)(LoopAttack(12, 7864.0, 1.0))
    assert lib.aware_embed_set_loop_attacks(sess.h, old, 1, seeds, C.c_void_p(ws.data_ptr()), big, None) == -1     # the older call
    nan, inf = float("nan"), float("inf")
    for p in ([-65537.0, 7864.0, 0.0, 0.0], [-7864.0, 65537.0, 0.0, 0.0], [7864.0, -7864.0, 0.0, 0.0], [-7864.5, 7864.0, 0.0, 0.0],
              [-7864.0, 7864.5, 0.0, 0.0], [nan, 7864.0, 0.0, 0.0], [-7864.0, nan, 0.0, 0.0], [-inf, 7864.0, 0.0, 0.0], [-7864.0, inf, 0.0, 0.0],
              [-7864.0, 7864.0, 1.0, 0.0], [-7864.0, 7864.0, 0.0, 1.0], [-7864.0, 7864.0, nan, 0.0], [-7864.0, 7864.0, 0.0, nan], WC[2], FB[2]):
        assert call([(12, 1.0, p)]) == -1, p
    assert call([(12, 1.5, FS[2])]) == -1 and call([(13, 1.0, FS[2])]) == -1
    assert call([FS, FS]) == -1 and call([FS, NO, FS]) == -1                                                        # a second entry
    for other in (RV, SP, ST, PS, PV, DS, FB, XC, WC):                                                              # forbidden neighbours
        assert call([FS, other]) == -1 and call([other, FS]) == -1, other
        assert call([other, NO, FS]) == -1 and call([FS, EV, other]) == -1, other
    assert call([ST, SP, FS]) == -1 and call([FS], n=5) == -1 and call([FS], sd=None) == -1
    assert call([FS], wsb=nb - 256) == -4 and call([NO, FS], wsb=nb - 256) == -4                                    # one 256-byte block short
    assert call([FS], wsb=nb) == 0 and lib.aware_embed_buffer(sess.h, 12) and not lib.aware_embed_buffer(sess.h, 13)     # the exact size
    assert call([], n=0) == 0 and not lib.aware_embed_buffer(sess.h, 12)
    assert call([NO, SU, FS, NO], wsb=nb) == 0 and call([EV, FS, EV, NO], wsb=nb) == 0
    assert call([(12, 0.0, [-65536.0, 65536.0, 0.0, 0.0])], wsb=nb) == 0 and call([(12, 1.0, [0.0, 0.0, 0.0, 0.0])], wsb=nb) == 0
    assert call([ST, SP]) == 0 and call([SP]) == 0 and call([RV]) == 0 and call([DS]) == 0 and call([FB]) == 0 and call([XC]) == 0
    assert call([FS], wsb=nb) == 0
    sess.iterate(1)
    torch.cuda.synchronize()
    assert call([FS]) == -1 and call([], n=0) == -1                        # after the first iterate
    with pytest.raises(ValueError):
        sess.set_loop_attacks([FSH], [1, 2])
    # the stand-alone entry, with real buffers: refused before anything is launched
    x = rt.Ragged.from_list([np.ones(2048, dtype=np.float32)])
    out = torch.empty(2048, device="cuda")
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    d, p0 = i32([0]), i32([0])
    p = lambda t: C.c_void_p(t.data_ptr())
    args = lambda **kw: [kw.get("inp", p(x.data)), p(x.d_off), p(x.d_len), kw.get("B", 1), kw.get("max_len", 2048), kw.get("d", p(d)), p(p0),
                         kw.get("adjoint", 0), kw.get("out", p(out)), None]
    assert lib.aware_frequency_shift(*args()) == 0
    for kw in (dict(B=0), dict(B=65536), dict(max_len=0), dict(max_len=(1 << 30) + 1), dict(adjoint=2), dict(adjoint=-1),
               dict(out=p(x.data)), dict(out=None), dict(inp=None), dict(d=None)):
        assert lib.aware_frequency_shift(*args(**kw)) == -1, kw
    torch.cuda.synchronize()
    assert torch.equal(out, x.data)


# ---- 6. card round trip -----------------------------------------------------------------------------------------------------------
def test_stereo_service_round_trip_with_the_card_key(rt, tmp_path):
    """load() of a card with the shift in loop_attacks, then embed_watermark / detect_watermark on a stereo clip: every channel
    carries the payload."""
    stereo_round_trip(tmp_path, "[{kind: frequency_shift, hz: 120.0, prob: 0.75}]", dict(FSH, prob=0.75))


# ---- 7. the value claim on the device ---------------------------------------------------------------------------------------------
def test_value_claim_on_the_device(rt, O, tmp_path):
    """The host test's two embeddings (four 1 s clips, seeds 0..3, 400 steps) through AWAREEmbedder(loop_attacks=...) from an
    edited card, under the host test's eight scipy.signal.hilbert shifts with its bounds: clean 0 % both, the plain mean over the
    eight at least 20 %, the aware mean at most a quarter of it.  Measured: plain 45 / 50 / 30 / 0 / 0 / 32.5 / 42.5 / 46.25 %,
    mean 30.78 %; aware 0 / 0 / 1.25 / 0 / 0 / 0 / 1.25 / 0 %, mean 0.31 %; clean 0 % for both; SNR 15.8 against 15.6 dB
    (DESIGN.md section 37)."""
    from test_loop_gain_host import snr_db
    from test_loop_shift_host import AWARE_CHAIN, hilbert_shifts
    clips, bits, embed, ber = value_claim_setup(O, tmp_path)

    y0, det = embed(None)
    y1, _ = embed(AWARE_CHAIN)
    y0, y1 = np.stack(y0), np.stack(y1)
    clean0, clean1 = ber(det, y0), ber(det, y1)
    b0 = {hz: ber(det, v) for hz, v in hilbert_shifts(y0).items()}
    b1 = {hz: ber(det, v) for hz, v in hilbert_shifts(y1).items()}
    for hz in b0:
        print(f"shift {hz:+6.0f} Hz   plain {b0[hz]:6.2f} %   shift-aware {b1[hz]:6.2f} %")
    m0, m1 = float(np.mean(list(b0.values()))), float(np.mean(list(b1.values())))
    audio = np.stack(clips)
    print(f"clean BER plain {clean0:.2f} % / shift-aware {clean1:.2f} %; mean over the eight: plain {m0:.2f} % / aware {m1:.2f} %; "
          f"SNR against the host: plain {snr_db(audio, y0):.1f} dB / aware {snr_db(audio, y1):.1f} dB")
    assert clean0 == 0.0 and clean1 == 0.0
    assert m0 >= 20.0
    assert m1 <= 0.25 * m0
