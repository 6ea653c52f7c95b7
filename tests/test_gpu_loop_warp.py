"""The time warp inside the embed loop (EXTENSION, chain kind 11) on the device: the kernels of csrc/loop_warp_kernels.hip -- the
table of rates and positions, the resampling and its gather-form adjoint -- alone and inside the loop, against the host twin
aware_amd/embedding/loop_attacks.py (warp_table, warp_positions, time_warp, time_warp_adjoint, apply_chain) composed with the
oracle's loop body.

The bounds of the operator alone are the ones tests/test_gpu_loop_speed.py derives for the same taps and the same weights, as a
fraction of each clip's reference peak, against the float64 twin on the same f32 operands.  Positions and fractions are integers,
exact on both sides, here as there (the table is compared bit for bit).  FORWARD: each weight is a cubic in Horner form, at most
four f32 roundings; the output sums four products (four more roundings) whose absolute values add up to at most 1.25 times the
input's peak: 8 * 2^-24 * 1.25 = 6e-7.  ADJOINT: an output gathers at most eight products (seven units of position at a step of
at least 58982 / 65536), so four roundings of a weight and eight of the sum; the weights that reach one output add up to at most
1.25 / 0.9 = 1.39 (the speed change's slowest rate is 0.794, hence its 1.26 * 1.25; this kind's is 0.9):
12 * 2^-24 * 1.39 = 9.9e-7, below the 1.05e-6 of the speed change's seven products at its wider weights.  CAP = 2e-6 is twice
that, for a reference peak below the operand's, and is the bound asserted for both directions; a larger error is a defect.

Inside the loop, buffer 12 is held to CHAIN_BOUND = 1.13e-6 of the peak, the loss and the prediction to 1e-5 and the
coefficient gradient to 2e-5 relative L2 per clip (2e-2 for at most one clip per case with a LeakyReLU argument within 1e-6 of
its kink): the tolerances of tests/test_gpu_loop_speed.py for the same quantities.

Shapes: stand-alone clips of 513, 4099, 7937, 16000 and 70000 samples packed back to back, so that all but the first start at odd
offsets; the last has 274 segments at e = 8, more than one chunk of the table's scan; one clip of 300000 samples has 1172, five
chunks.  Sessions: clips of 16128 and 16384 samples (64 and 65 frames; 63 and 64 hop blocks).

Run on the MI355X box:  python -m pytest tests/test_gpu_loop_warp.py -m gpu -q -s"""
import ctypes as C

import numpy as np
import pytest
import torch

from loop_support import CHAIN_BOUND, DS, EV, FB, LA, NO, NOISE10, O, PS, PV, RV, SP, ST, SU, SUP, WC, XC, attacked, bits_equal
from loop_support import ex_entries, first_gradient, forward_at_run_length, mixture_is_its_chains, norm2
from loop_support import prob_0_is_the_plain_loop, rt, sampled, session, step_0_is_the_stand_alone_entry, synthesis
from loop_support import value_claim_setup

pytestmark = pytest.mark.gpu

RAGGED = [16128, 16384]                                    # 64 and 65 frames
TW = {"kind": "time_warp", "depth": 0.04, "period": [0.032, 0.512]}
ENV = {"kind": "gain_envelope", "period": [0.05, 0.5], "floor": 0.25}
CHAINS = {"warp": [TW], "noise_warp_noise": [NOISE10, TW, NOISE10], "envelope_warp_suppression": [ENV, TW, SUP]}
KINK = 1e-6                                                # the speed change's rule, not the pv rule's 8e-6
CAP = 2e-6                                                 # derived above
assert CHAIN_BOUND == 1.13e-6
ALONE = [513, 4099, 7937, 16000, 70000]


def drawn(LA, chain, seed, step, ny):
    """(fires, e, ph, rate offsets) of the chain's time warp for this clip at this step."""
    chain = LA.parse_chain(chain)
    j = [a["kind"] for a in chain].index("time_warp")
    r = LA.entry_draw(seed, step, j)
    e, ph = LA.warp_draw(chain[j], r, 16000)
    m = LA.warp_rates(seed, step, j, LA.warp_breakpoints(ny, e), LA.warp_range(chain[j], 16000)[2])
    return LA.fires(r[0], chain[j]["prob"]), e, ph, m


# ---- 1. the operator alone ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def alone():
    """Five clips and the float64 reference of every case, computed once: {(e, end, D): per clip (ph, m, z, gx)} with the gradient
    g = 0.5 z + 0.5 noise in f32, so that <z, g> is about half of |z|^2: well away from zero."""
    from aware_amd.embedding import loop_attacks as LA
    rng = np.random.default_rng(31)
    xs = [rng.standard_normal(n).astype(np.float32) for n in ALONE]
    ns = [rng.standard_normal(n).astype(np.float32) for n in ALONE]
    cases = {}
    for e in (8, 10, 14):
        for end in (0, 1):
            for D in (1, 6553):
                per = []
                for b, (x, noise) in enumerate(zip(xs, ns)):
                    ph = end * ((1 << e) - 1)
                    m = LA.warp_rates(100 * e + b, end, 0, LA.warp_breakpoints(len(x), e), D)
                    z = LA.time_warp(torch.from_numpy(x).double(), e, ph, m)
                    g = (0.5 * z.float() + 0.5 * torch.from_numpy(noise)).numpy()
                    gx = LA.time_warp_adjoint(torch.from_numpy(g).double(), e, ph, m)
                    per.append((ph, m, z.numpy(), g, gx.numpy()))
                cases[(e, end, D)] = per
    return xs, cases


def check_table(LA, tr, ta, es, ms, counts):
    for b, (e, m, c) in enumerate(zip(es, ms, counts)):
        R, A = LA.warp_table(m[:c], e)
        assert np.array_equal(tr[b, :c].cpu().numpy().astype(np.int64), R) and np.array_equal(ta[b, :c].cpu().numpy(), A), b


@pytest.mark.parametrize("D", [1, 6553])
@pytest.mark.parametrize("end", [0, 1], ids=["ph0", "phP-1"])
@pytest.mark.parametrize("e", [8, 10, 14])
def test_time_warp_against_the_host_twin(rt, LA, alone, e, end, D):
    """aware_time_warp, forward and adjoint, on the ragged batch (the second clip starts at float offset 513), against the
    float64 twin within CAP of each clip's reference peak; the table (R_k, A(k)) the device built equals the host's bit for bit,
    and the adjoint gives the same bits from the device's table and from the host's; exact zeros where the twin has none of the
    clip left; <z, g> = <x, gx> on the device's results to 1e-6 relative, summed in float64."""
    xs, cases = alone
    per = cases[(e, end, D)]
    phs, ms = [p[0] for p in per], [p[1] for p in per]
    x = rt.Ragged.from_list(xs)
    assert list(x.offsets[:3]) == [0, 513, 4612]
    z, tr, ta = rt.time_warp(x, e, phs, ms, return_table=True)
    counts = [LA.warp_breakpoints(n, e) for n in ALONE]
    assert tuple(tr.shape) == (5, max(counts)) and (e != 8 or counts[-1] - 1 == 275 > 256)
    check_table(LA, tr, ta, [e] * 5, ms, counts)
    g = rt.Ragged.from_list([p[3] for p in per])
    gx = rt.time_warp(g, e, phs, ms, adjoint=True, table=(tr, ta))
    gx_host = rt.time_warp(g, e, phs, ms, adjoint=True)
    assert torch.equal(gx.data, gx_host.data)
    worst_f = worst_a = worst_ip = 0.0
    for xi, zi, gxi, (ph, m, ref, gi, refg) in zip(xs, z.to_list(), gx.to_list(), per):
        n = len(xi)
        worst_f = max(worst_f, np.abs(zi - ref).max() / np.abs(ref).max())
        worst_a = max(worst_a, np.abs(gxi - refg).max() / np.abs(refg).max())
        dead = LA.warp_positions(n, e, ph, m) > ((n - 1) << 16)
        assert np.all(zi[dead] == 0.0) and np.array_equal(dead, np.sort(dead))              # zeros at the end only
        a, b = float(np.dot(zi.astype(np.float64), gi.astype(np.float64))), float(np.dot(xi.astype(np.float64), gxi.astype(np.float64)))
        assert a > 0.25 * float(np.dot(ref, ref))
        worst_ip = max(worst_ip, abs(a - b) / abs(a))
    print(f"time_warp e = {e}, ph = {phs[0]}, D = {D}: max error / peak forward {worst_f:.2e}, adjoint {worst_a:.2e}; "
          f"|<z, g> - <x, gx>| / <z, g> = {worst_ip:.2e}")
    assert worst_f < CAP and worst_a < CAP, (worst_f, worst_a)
    assert worst_ip < 1e-6, worst_ip


def test_a_long_clip_scans_across_chunks(rt, LA):
    """One clip of 300000 samples at e = 8: 1174 breakpoints, five chunks of the table's scan with a carry between them; the
    table bit for bit, both directions within CAP, the inner product to 1e-6."""
    rng = np.random.default_rng(37)
    n = 300000
    xi = rng.standard_normal(n).astype(np.float32)
    m = LA.warp_rates(9, 0, 0, LA.warp_breakpoints(n, 8), 6553)
    assert len(m) == 1174
    z, tr, ta = rt.time_warp(rt.Ragged.from_list([xi]), 8, 77, [m], return_table=True)
    check_table(LA, tr, ta, [8], [m], [1174])
    ref = LA.time_warp(torch.from_numpy(xi).double(), 8, 77, m)
    gi = (0.5 * ref.float() + 0.5 * torch.from_numpy(rng.standard_normal(n).astype(np.float32))).numpy()
    refg = LA.time_warp_adjoint(torch.from_numpy(gi).double(), 8, 77, m).numpy()
    gx = rt.time_warp(rt.Ragged.from_list([gi]), 8, 77, [m], adjoint=True, table=(tr, ta)).to_list()[0]
    zi, ref = z.to_list()[0], ref.numpy()
    ef, ea = np.abs(zi - ref).max() / np.abs(ref).max(), np.abs(gx - refg).max() / np.abs(refg).max()
    a, b = float(np.dot(zi.astype(np.float64), gi.astype(np.float64))), float(np.dot(xi.astype(np.float64), gx.astype(np.float64)))
    print(f"300000 samples at e = 8: max error / peak forward {ef:.2e}, adjoint {ea:.2e}; inner products differ by {abs(a - b) / abs(a):.2e}")
    assert ef < CAP and ea < CAP and abs(a - b) < 1e-6 * abs(a)


def test_constant_rates_and_errors(rt, LA):
    """All-zero offsets copy the clip bit for bit in both directions; all +D and all -D are the speed change at m = +-D, whose
    stand-alone kernel runs the same taps: bit for bit, both directions, +D ending in exact zeros.  A clip alone gives the same
    bits as inside a batch, wherever it starts.  runtime.time_warp refuses what the twin refuses."""
    rng = np.random.default_rng(41)
    lengths = [513, 4099, 7937]
    xs = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    x = rt.Ragged.from_list(xs)
    for e in (8, 10, 14):
        K = [LA.warp_breakpoints(n, e) for n in lengths]
        for ph in (0, (1 << e) - 1):
            zero = [np.zeros(k, dtype=np.int64) for k in K]
            for adjoint in (False, True):
                assert torch.equal(rt.time_warp(x, e, ph, zero, adjoint=adjoint).data, x.data)
            for D in (1, 6553):
                for sign in (1, -1):
                    m = [np.full(k, sign * D, dtype=np.int64) for k in K]
                    for adjoint in (False, True):
                        got = rt.time_warp(x, e, ph, m, adjoint=adjoint)
                        want = rt.speed_change(x, sign * D, adjoint=adjoint, out_lengths=lengths)
                        assert torch.equal(got.data, want.data), (e, ph, D, sign, adjoint)
            fast = rt.time_warp(x, e, ph, [np.full(k, 6553, dtype=np.int64) for k in K]).to_list()
            for zi, n in zip(fast, lengths):
                live = LA.speed_length(n, 6553)
                assert live < n and np.all(zi[live:] == 0.0) and zi[live - 1] != 0.0
    ms = [LA.warp_rates(b, 0, 0, LA.warp_breakpoints(n, 8), 3000) for b, n in enumerate(lengths)]
    both = rt.time_warp(x, 8, [0, 100, 255], ms).to_list()
    for xi, zi, ph, m in zip(xs, both, (0, 100, 255), ms):
        assert bits_equal(rt.time_warp(rt.Ragged.from_list([xi]), 8, ph, [m]).to_list()[0], zi)
    for bad in ((8, 0, ms[:2]), (7, 0, ms), (21, 0, ms), (8, 256, ms), (8, -1, ms), (8, 0, [m[:-1] for m in ms]),
                (8, 0, [np.full(len(m), 6554) for m in ms]), ([8, 8], 0, ms)):
        with pytest.raises(ValueError):
            rt.time_warp(x, *bad)
    from aware_amd import attacks as A
    out = A.TimeWarp(depth=0.04, seed=3).apply_batch(x, 16000).to_list()
    e1, ph1 = LA.warp_draw(LA.parse_chain([TW])[0], LA.entry_draw(4, 0, 0), 16000)
    want = rt.time_warp(rt.Ragged.from_list([xs[1]]), e1, ph1, [LA.warp_rates(4, 0, 0, LA.warp_breakpoints(4099, e1), 2621)]).to_list()[0]
    assert bits_equal(out[1], want)
    fl = A.Flutter(0.03, 6.0, 2.0)
    assert bits_equal(fl.apply(xs[2], 16000), rt.time_warp(rt.Ragged.from_list([xs[2]]), 8, 0, [fl.rates(7937, 16000)]).to_list()[0])


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
def test_forward_matches_the_restatement(rt, O, LA, name):
    """Buffer 12 against apply_chain(N(N(buffer 9))) at steps 0, 2 and 17 on the ragged session of 64 and 65 frames, within
    CHAIN_BOUND = 1.13e-6 of the peak; the draws differ from step to step."""
    chain = LA.parse_chain(CHAINS[name])
    seeds = [11, 14]
    sess, batch, _, _ = session(rt, O, RAGGED, [20, 21], chain, seeds, num_iterations=20)
    assert batch.out_lengths == [16128, 16384]
    sess.gradient()
    check_forward(LA, sess, batch, chain, seeds, 0, name)
    sess.iterate(3)
    check_forward(LA, sess, batch, chain, seeds, 2, name)
    sess.iterate(15)
    assert int(sess.step.cpu()[0]) == 18
    check_forward(LA, sess, batch, chain, seeds, 17, name)
    assert len({tuple(drawn(LA, chain, seeds[0], s, 16128)[3][:3].tolist()) for s in (0, 2, 17)}) == 3


def test_step_0_is_the_stand_alone_entry(rt, O, LA):
    """Buffer 12 at step 0 is aware_time_warp with the host's draw on the same input, bit for bit: the loop's kernels and the
    stand-alone ones share their arithmetic, and the table kernel's draws are the host's.  The input x = N(N(y)) in the device's
    own rounding is buffer 12 of a second session whose entry never fires, which is therefore a copy."""
    def alone(x):
        d = [drawn(LA, [TW], sd, 0, n) for sd, n in zip([3, 4], x.lengths)]
        assert all(v[0] for v in d)
        return rt.time_warp(x, [v[1] for v in d], [v[2] for v in d], [v[3] for v in d])

    step_0_is_the_stand_alone_entry(rt, O, RAGGED, TW, alone)


# ---- 3. first gradient ----------------------------------------------------------------------------------------------------------
# First clip seed of each case, chosen on the CPU (oracle only) so that the float64 composition keeps every LeakyReLU argument of
# both clips at least 1e-5 from its kink, the first such seed from 80 on: warp 80 (1.2e-5 / 1.3e-4), noise_warp_noise 81
# (4.5e-5 / 2.6e-5; 80 had a clip at 9.1e-6), envelope_warp_suppression 80 (1.6e-5 / 6.8e-5).  The check below still allows one
# clip per case within KINK at 2e-2, as the speed change's does, and prints the distances.
SEED0 = {"warp": 80, "noise_warp_noise": 81, "envelope_warp_suppression": 80}


def check_first_gradient(rt, O, LA, chain, lengths, clip_seed0, **kw):
    batch, seeds, figures = first_gradient(rt, O, LA, chain, lengths, list(range(clip_seed0, clip_seed0 + len(lengths))), **kw)
    near = 0
    for i, (rel, kink, lerr, perr) in enumerate(figures):
        near += int(kink <= KINK)
        on, e, ph, m = drawn(LA, chain, seeds[i], 0, batch.out_lengths[i])
        print(f"{kw} clip {i} (n = {lengths[i]}, fires {on}, e = {e}, ph = {ph}): loss err {lerr:.1e}, pred err {perr:.1e}, "
              f"gradient rel L2 {rel:.2e}, nearest LeakyReLU kink {kink:.1e}")
        assert on, "the case is to exercise the operator"
        assert lerr < 1e-5 and perr < 1e-5, (i, lerr, perr)
        assert rel < (2e-5 if kink > KINK else 2e-2), (i, rel, kink)
    assert near <= 1, near


@pytest.mark.parametrize("name", list(CHAINS))
@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
def test_first_gradient(rt, O, LA, name, dsp_path):
    """aware_embed_gradient against torch autograd over the restatement composed with the oracle's loop body, with the rule and
    the tolerances of tests/test_gpu_loop_speed.py: 2e-5 relative L2 per clip (2e-2 for at most one clip per case with a
    LeakyReLU argument within 1e-6 of its kink), loss and prediction 1e-5."""
    check_first_gradient(rt, O, LA, CHAINS[name], RAGGED, SEED0[name], dsp_path=dsp_path)


# ---- 4. per-clip and replay behaviour ---------------------------------------------------------------------------------------------
def test_prob_0_is_the_plain_loop(rt, O):
    """A time warp that never fires against the loop without a chain: coefficients, best coefficients and losses after 20 steps
    and the gradient of step 20, bit for bit, alone and between two older entries that never fire either, on both dsp_paths."""
    prob_0_is_the_plain_loop(rt, O, ([dict(TW, prob=0.0)], [dict(SUP, prob=0.0), dict(TW, prob=0.0), dict(NOISE10, prob=0.0)]),
                             lengths=[8000, 16128, 16384])


def test_a_clip_that_does_not_fire_keeps_its_bits(rt, O, LA):
    """prob 0.5 on three clips, 8 steps: where the entry does not fire, buffer 12 is buffer 12 of a session whose entry never
    fires, N(N(buffer 9)) in the device's rounding, bit for bit (checked at step 0, where the two sessions hold the same
    coefficients), and within 2e-7 of the float64 value at every step; where it fires it is the warp of that within CHAIN_BOUND.
    Both occur."""
    lengths, seeds = [16128, 8000, 16384], [1, 2, 3]
    chain = LA.parse_chain([dict(TW, prob=0.5)])
    sess, batch, _, _ = session(rt, O, lengths, [70, 71, 72], chain, seeds, num_iterations=20)
    never, _, _, _ = session(rt, O, lengths, [70, 71, 72], [dict(TW, prob=0.0)], seeds, num_iterations=20)
    never.gradient()
    seen = set()
    for step in range(8):
        sess.iterate(1)
        torch.cuda.synchronize()
        for b, (y, z) in enumerate(zip(synthesis(sess, batch), attacked(sess, batch))):
            on = drawn(LA, chain, seeds[b], step, len(y))[0]
            seen.add(on)
            if on:
                ref = LA.apply_chain(norm2(y.double())[None], [TW], [seeds[b]], step)[0]
                assert float((z.double() - ref).abs().max() / ref.abs().max()) < CHAIN_BOUND, (step, b)
            else:
                assert float((z.double() - norm2(y.double())).abs().max()) < 2e-7, (step, b)
                if step == 0:
                    assert torch.equal(z, attacked(never, batch)[b])
    assert seen == {False, True}


def test_graph_replay_redraws_every_step(rt, O, LA):
    """Under graph replay and without it: the same bits; and two consecutive replayed steps draw different warps, each buffer 12
    the host's warp for its own step of its own buffer 9, within CHAIN_BOUND."""
    chain = LA.parse_chain([TW])
    seeds = [0, 1]
    out = []
    for use_graph in (True, False):
        sess, batch, _, _ = session(rt, O, RAGGED, [50, 51], chain, seeds, num_iterations=12, use_graph=use_graph)
        sess.iterate(4)
        zs = []
        for step in range(4, 8):
            sess.iterate(1)
            if use_graph:
                check_forward(LA, sess, batch, chain, seeds, step, "replay")
            zs.append(sess.attacked.clone())
        torch.cuda.synchronize()
        out.append((sess.coef.cpu(), sess.best_coef.cpu(), sess.loss.cpu(), torch.stack(zs).cpu()))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    d = [drawn(LA, chain, 0, s, 16128) for s in range(4, 8)]
    assert len({(v[1], v[2], tuple(v[3][:4].tolist())) for v in d}) == 4


def test_a_mixture_is_its_chains(rt, O, LA):
    """A mixture of {time warp, noise} and {reverberation} at step 0: buffer 14 holds the host's choices, and every clip's buffer
    12 (with buffer 9, loss, prediction and its rows of the coefficient gradient) is bit for bit that of a session that holds only
    the chain the clip drew; the clips of the warp chain are within CHAIN_BOUND of the float64 restatement."""
    mixture_is_its_chains(rt, O, LA, [TW, NOISE10], [{"kind": "reverberation", "rt60": [0.1, 0.3]}], lengths=[16128, 8000, 16384, 8000],
                          bound=CHAIN_BOUND)


@pytest.mark.parametrize("bname", ["R12", "R8", "R6"])
def test_forward_at_every_synthesis_run_length(rt, O, LA, bname):
    """The batches of tests/test_loop_run_rule_host.py that select synthesis runs of 12, 8 and 6 hop blocks (every other session of
    this module runs at 4): buffer 12 of the five head clips (18432, 16000, 8000, 24000 and 513 samples) at steps 0 and 2 within
    CHAIN_BOUND of the restatement on N(N(buffer 9)).  A workgroup's share of a clip then spans up to 3072 samples, several
    segments of the finest period."""
    forward_at_run_length(rt, O, LA, bname, "warp", LA.parse_chain([TW]), check_forward)


# ---- 5. workspace and error codes -------------------------------------------------------------------------------------------------
def test_entry_point_error_codes(rt, O, LA):
    from aware_amd._lib import LoopAttack
    sess, batch, _, _ = session(rt, O, RAGGED, [64, 65], None, num_iterations=20, use_graph=False)
    lib = sess.lib
    size = lambda ent: lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries(ent), len(ent))
    nb = size([WC])
    # the deletion twin's bytes and the two tables, int [B][K] and long long [B][K], each at the next 256-byte boundary
    al = lambda v: (v + 255) & ~255
    K = LA.warp_breakpoints(16384, 9)
    assert nb == al(al(size([DS])) + 4 * 2 * K) + 8 * 2 * K and size([NO, SU, WC, NO]) - size([NO, SU, DS, NO]) == nb - size([DS])
    for other in (RV, SP, ST, PS, PV, DS, FB, XC):                                                                  # a refused pair: the older kind's bytes
        assert size([WC, other]) == size([other, WC]) == size([other])
    big = max(nb, size([RV]), size([PV])) + 8 * batch.total_out + 512
    ws = torch.empty(big, dtype=torch.uint8, device="cuda")
    seeds = (C.c_uint32 * 2)(1, 2)
    assert batch.out_lengths == [16128, 16384]

    def call(entries, n=None, wsb=big, sd=seeds):
        return lib.aware_embed_set_loop_attacks_ex(sess.h, ex_entries(entries), len(entries) if n is None else n, sd,
                                                   C.c_void_p(ws.data_ptr()), wsb, None)

    old = (LoopAttack * 1)(LoopAttack(11, 9.0, 1.0))
    assert lib.aware_embed_set_loop_attacks(sess.h, old, 1, seeds, C.c_void_p(ws.data_ptr()), big, None) == -1     # the older call
    nan, inf = float("nan"), float("inf")
    for p in ([7.0, 13.0, 2621.0, 0.0], [0.0, 13.0, 2621.0, 0.0], [-9.0, 13.0, 2621.0, 0.0], [9.5, 13.0, 2621.0, 0.0],
              [9.0, 13.5, 2621.0, 0.0], [13.0, 9.0, 2621.0, 0.0], [9.0, 21.0, 2621.0, 0.0], [9.0, 13.0, 0.0, 0.0], [9.0, 13.0, -1.0, 0.0],
              [9.0, 13.0, 6554.0, 0.0], [9.0, 13.0, 2621.5, 0.0], [9.0, 13.0, 2621.0, 1.0], [nan, 13.0, 2621.0, 0.0], [9.0, nan, 2621.0, 0.0],
              [9.0, inf, 2621.0, 0.0], [9.0, 13.0, nan, 0.0], [9.0, 13.0, 2621.0, nan], FB[2], XC[2], [0.0]):
        assert call([(11, 1.0, p)]) == -1, p
    assert call([(11, 1.5, WC[2])]) == -1 and call([(12, 1.0, WC[2])]) == -1
    assert call([WC, WC]) == -1 and call([WC, NO, WC]) == -1                                                        # a second entry
    for other in (RV, SP, ST, PS, PV, DS, FB, XC):                                                                  # forbidden neighbours
        assert call([WC, other]) == -1 and call([other, WC]) == -1, other
        assert call([other, NO, WC]) == -1 and call([WC, EV, other]) == -1, other
    assert call([ST, SP, WC]) == -1 and call([WC], n=5) == -1 and call([WC], sd=None) == -1
    assert call([WC], wsb=nb - 256) == -4 and call([NO, WC], wsb=nb - 256) == -4                                    # 256 bytes short
    assert call([WC], wsb=nb) == 0 and lib.aware_embed_buffer(sess.h, 12) and not lib.aware_embed_buffer(sess.h, 13)     # the exact size
    assert call([], n=0) == 0 and not lib.aware_embed_buffer(sess.h, 12)
    assert call([NO, SU, WC, NO], wsb=nb) == 0 and call([EV, WC, EV, NO], wsb=nb) == 0
    assert call([(11, 0.0, [8.0, 8.0, 1.0, 0.0])], wsb=size([(11, 0.0, [8.0, 8.0, 1.0, 0.0])])) == 0
    assert call([(11, 1.0, [8.0, 20.0, 6553.0, 0.0])], wsb=nb) == -4 and call([(11, 1.0, [20.0, 20.0, 6553.0, 0.0])], wsb=nb) == 0      # sized from e_lo
    assert call([ST, SP]) == 0 and call([SP]) == 0 and call([RV]) == 0 and call([DS]) == 0 and call([FB]) == 0 and call([XC]) == 0
    assert call([WC], wsb=nb) == 0
    sess.iterate(1)
    torch.cuda.synchronize()
    assert call([WC]) == -1 and call([], n=0) == -1                        # after the first iterate
    with pytest.raises(ValueError):
        sess.set_loop_attacks([TW], [1, 2])
    # the stand-alone entry, with real buffers: refused before anything is launched
    x = rt.Ragged.from_list([np.ones(2048, dtype=np.float32)])
    out = torch.empty(2048, device="cuda")
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    e, ph, m, tr, ta = i32([8]), i32([0]), i32([0] * 10), i32([0] * 10), torch.zeros(10, dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    args = lambda **kw: [kw.get("inp", p(x.data)), p(x.d_off), p(x.d_len), kw.get("B", 1), kw.get("max_len", 2048), p(e), p(ph), p(m),
                         kw.get("stride", 10), kw.get("tr", p(tr)), p(ta), kw.get("out", p(out)), kw.get("adjoint", 0), None]
    assert lib.aware_time_warp(*args()) == 0
    for kw in (dict(B=0), dict(B=65536), dict(max_len=0), dict(max_len=(1 << 30) + 1), dict(stride=2), dict(adjoint=2), dict(adjoint=-1),
               dict(out=p(x.data)), dict(out=None), dict(inp=None), dict(tr=None)):
        assert lib.aware_time_warp(*args(**kw)) == -1, kw
    torch.cuda.synchronize()
    assert torch.equal(out, x.data)


# ---- 6. the value claim on the device ---------------------------------------------------------------------------------------------
def test_value_claim_on_the_device(rt, O, tmp_path):
    """The host test's three embeddings (four 1 s clips, seeds 0..3, 400 steps) through AWAREEmbedder(loop_attacks=...) from an
    edited card, attacked on the host with the host test's eight flutters (scipy's cubic spline) and read on the device, with its
    bounds: clean 0 % for all three, the plain mean at least 10 %, the warp-aware mean at most half of it and below the
    speed-aware mean.  Measured: means 40.62 / 16.41 / 5.00 % at depth 0.03, every cell 0 % at depth 0.01 (printed), clean 0 %,
    SNR 15.8 / 15.2 / 15.1 dB; the cells are in DESIGN.md section 35."""
    from test_loop_warp_host import AWARE_CHAIN, SPEED_CHAIN, flutter_table, report
    from test_loop_gain_host import snr_db
    clips, bits, embed, _ = value_claim_setup(O, tmp_path)

    ys, det = [], None
    for chain in (None, SPEED_CHAIN, AWARE_CHAIN):
        y, det = embed(chain)
        ys.append(np.stack(y))

    def read(z):
        vals = det.detect_batch(list(z), 16000).cpu().numpy()
        return 100.0 * float((O.decode_bits(vals) != bits).mean())

    names, audio = ["plain", "speed-aware", "warp-aware"], np.stack(clips)
    clean, snr = [read(y) for y in ys], [snr_db(audio, y) for y in ys]
    report(names, [flutter_table(read, y, 0.01) for y in ys], clean, snr, 0.01)
    m0, m1, m2 = report(names, [flutter_table(read, y, 0.03) for y in ys], clean, snr, 0.03)
    assert clean == [0.0, 0.0, 0.0]
    assert m0 >= 10.0
    assert m2 <= 0.5 * m0
    assert m2 < m1
