"""What the loop-attack device tests (tests/test_gpu_loop_*.py) share, each stated once: the rt / O / LA fixtures, the session
helpers, the constants that mean one thing across the family, and the bodies of the checks that every kind's module repeats with
its own entry, draw function and seeds.  The functions here are not tests.  A kind's module keeps its `def test_...` with its
docstring, its recorded seeds and figures and its kind-specific second half, and calls in here with its own pieces as arguments
(DESIGN.md section 26).

pytest does not rewrite the asserts of a module that is not named test_*.py, so every assert in this file carries its own
message: the values it compared.

A value that differs between modules is not here: it stays in its module, under the module's own name (the filter's SUP of
0.02 s, the KINK = 1e-6 of the speed change and the time warp, every RAGGED other than [16000, 8000])."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, make_clip


# ---- fixtures: import them by name ------------------------------------------------------------------------------------------------
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


# ---- constants --------------------------------------------------------------------------------------------------------------------
CHAIN_BOUND = 1.13e-6       # the project's bound for the loop's attacked signal, of the reference's peak (measured in
#                             tests/test_gpu_loop_reverb.py)
KINK = 8e-6                 # the pv rule's least distance of a LeakyReLU argument from its kink, in float64 and in float32
NOISE10 = {"kind": "gaussian_noise", "snr_db": 10.0}
SUP = {"kind": "sample_suppression", "seconds": 0.3}
SHORT, LONG, RAGGED = [8000] * 2, [16000] * 2, [16000, 8000]

# C ABI entries (kind, prob, parameters), one per kind
NO = (0, 1.0, [10.0])
SU = (1, 1.0, [4800.0])
RV = (2, 1.0, [1600.0, 8000.0, -3.0])
SP = (3, 0.75, [-3678.0, 3896.0])
ST = (4, 0.75, [-9830.0, 9830.0])
PS = (5, 0.75, [-3678.0, 3896.0])
PV = (6, 0.9, [-9830.0, 9830.0, -5435.0, 5930.0])
DS = (7, 0.75, [1.0, 512.0, 0.0])
EV = (8, 0.75, [800.0, 8000.0, 0.25])
FB = (9, 0.75, [15.0, 2458.0, 15565.0, 1638.0])
XC = (10, 0.75, [3000.0, 10000.0, 0.0, 0.0])
WC = (11, 0.75, [9.0, 13.0, 2621.0, 0.0])
# aware_embed_loop_attack_workspace_bytes_ex for the batch [16000, 8000], computed with the library of the commit before the
# time stretch: chains without a newer kind need exactly these
PARENT_WORKSPACE = {"noise": 104968, "noise_suppression": 104968, "reverb": 685824, "suppression_reverb_noise": 685824,
                    "speed": 200448, "noise_speed": 200448, "four": 200448}


def ex_entries(entries):
    from aware_amd._lib import LoopAttackEx
    return (LoopAttackEx * max(1, len(entries)))(*[LoopAttackEx(k, pr, (C.c_float * 4)(*(list(p) + [0.0] * (4 - len(p)))))
                                                   for k, pr, p in entries])


# ---- sessions and their buffers -----------------------------------------------------------------------------------------------------
_PLANS, _DETS = {}, {}


def plan_for(rt, band=(32, 256)):
    if band not in _PLANS:
        _PLANS[band] = rt.Plan(band_bins=band)
    return _PLANS[band]


def det_for(rt, O, band=(32, 256)):
    if band not in _DETS:
        ws, bs = O.detector_weights()
        _DETS[band] = rt.DetectorWeights(plan_for(rt, band), O.mel_filter_bank(), [w.numpy() for w in ws], [b.numpy() for b in bs])
    return _DETS[band]


def session(rt, O, lengths, seeds, chain=None, attack_seeds=None, band=(32, 256), **kw):
    pairs = [make_clip(s, n) for s, n in zip(seeds, lengths)]
    wm = np.stack([O.bits_to_bipolar(p[1]) for p in pairs]).astype(np.float32)
    batch = rt.Batch(lengths)
    sess = rt.EmbedSession(plan_for(rt, band), det_for(rt, O, band), batch, **kw)
    if chain is not None:
        sess.set_loop_attacks(chain, attack_seeds if attack_seeds is not None else list(range(len(lengths))))
    sess.begin(batch.pack([p[0] for p in pairs]), torch.from_numpy(wm).cuda())
    return sess, batch, pairs, wm


def norm2(y):
    """N(N(y)) as the kernels apply it in front of the chain."""
    y = y / (y.abs().max() + 1e-8)
    return y / (y.abs().max() + 1e-8)


def synthesis(sess, batch):
    y = sess._view(9, (batch.total_out,)).cpu()
    return [y[o:o + n] for o, n in zip(batch.out_offsets, batch.out_lengths)]


def attacked(sess, batch):
    z = sess.attacked.cpu()
    return [z[o:o + n] for o, n in zip(batch.out_offsets, batch.out_lengths)]


def sampled(sess, batch, sample=None):
    """(b, buffer 9, buffer 12) of every clip, or of the clips `sample` names only (a batch whose other clips are filler)."""
    ys, zs = synthesis(sess, batch), attacked(sess, batch)
    return [(b, ys[b], zs[b]) for b in (range(batch.B) if sample is None else sample)]


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def plus_zero(a):
    """a with every -0.0 turned into +0.0 and every other bit kept (x + 0.0 in round-to-nearest).  The restatement suppresses by
    multiplying with a 0/1 mask, which leaves -0.0 under a negative sample; the device writes +0.0.  The sign of a suppressed
    zero is no part of the model."""
    return np.ascontiguousarray(a, dtype=np.float32) + np.float32(0.0)


def device_x(y):
    """x = N(N(y)) in the device's own rounding (csrc/common.hpp clip_norm_from_partials, chain_kernel): float32 throughout,
    m = max|y| + 1e-8, m2 = max|y| / m + 1e-8, x = (y * (1 / m)) * (1 / m2)."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    raw = np.float32(np.abs(y).max())
    m = np.float32(raw + np.float32(1e-8))
    m2 = np.float32(np.float32(raw / m) + np.float32(1e-8))
    return ((y * np.float32(np.float32(1.0) / m)) * np.float32(np.float32(1.0) / m2)).astype(np.float32)


# the sessions of the mixture tests: the same clips for a mixture, for one of its chains and for no chain
_CLIPS = {}


def clips_for(O, lengths):
    key = tuple(lengths)
    if key not in _CLIPS:
        pairs = [make_clip(200 + i, n) for i, n in enumerate(lengths)]
        _CLIPS[key] = ([p[0] for p in pairs], np.stack([O.bits_to_bipolar(p[1]) for p in pairs]).astype(np.float32))
    return _CLIPS[key]


def mixture_session(rt, O, lengths, seeds=None, mixture=None, chain=None, **kw):
    """A session on the shared clips of these lengths, begun, with a mixture, a chain or neither."""
    audio, wm = clips_for(O, lengths)
    batch = rt.Batch(lengths)
    sess = rt.EmbedSession(plan_for(rt), det_for(rt, O), batch, **kw)
    if mixture is not None:
        sess.set_loop_mixture(mixture, seeds)
    elif chain is not None:
        sess.set_loop_attacks(chain, seeds)
    sess.begin(batch.pack(audio), torch.from_numpy(wm).cuda())
    return sess, batch


def weights(mixture):
    return [m["weight"] for m in mixture]


def rows(batch, b):
    return slice(batch.frame_offsets[b], batch.frame_offsets[b + 1])


def span(batch, b):
    return slice(batch.out_offsets[b], batch.out_offsets[b] + batch.out_lengths[b])


# ---- the oracle's loop body with a chain in it ----------------------------------------------------------------------------------------
def attacked_oracle(O, LA, chain, seed, step=0, band=None, dtype=None):
    class Attacked(O.Embedder):
        def recompute_magnitude(self, mag_full, phase):
            y = O.istft(mag_full * torch.exp(1j * phase))
            y = y / torch.amax(torch.abs(y) + 1e-8, dim=-1, keepdim=True)
            y = y / torch.amax(torch.abs(y) + 1e-8, dim=-1, keepdim=True)
            y = LA.apply_chain(y, chain, [seed], step)
            y = y / torch.amax(torch.abs(y) + 1e-8, dim=-1, keepdim=True)
            y = y / torch.amax(torch.abs(y) + 1e-8, dim=-1, keepdim=True)
            return torch.abs(O.stft(y)), y
    emb = Attacked() if dtype is None else Attacked(dtype=dtype)
    if band is not None:
        emb.band, emb.nonband = O.band_indices(bands=(band[0] * 15.625, band[1] * 15.625))
    return emb


def oracle_gradient(O, LA, chain, seed, clip, wm, dtype):
    """Gradient, loss, prediction and the nearest LeakyReLU kink of the composition at step 0, in this precision."""
    from test_gpu_kernels import _min_kink_distance
    emb = attacked_oracle(O, LA, chain, seed, 0, dtype=dtype)
    mag0, phase = emb.analyse(torch.from_numpy(clip).to(dtype)[None])
    c0 = mag0[:, emb.band].clone().requires_grad_(True)
    l, p = emb.forward_loss(c0, mag0, phase, torch.from_numpy(wm).to(dtype)[None])
    l.sum().backward()
    return c0.grad[0].double(), float(l.detach()), p[0].detach().double().numpy(), _min_kink_distance(emb, mag0, phase)


# ---- forward --------------------------------------------------------------------------------------------------------------------------
def forward_at_steps_0_2_17(rt, O, LA, chain, lengths, tag, check_forward, shortest=(7936, 15872)):
    """A session of 20 steps on clips 20, 21, ... with attack seeds 11, 14, ...: the module's check_forward of buffer 12 at step
    0 (after gradient()), at step 2 (after three steps) and at step 17 (after eighteen).  Returns the batch and the attack seeds,
    for the module's own check that the draws differ from step to step."""
    seeds = [11 + 3 * i for i in range(len(lengths))]
    sess, batch, _, _ = session(rt, O, lengths, list(range(20, 20 + len(lengths))), chain, seeds, num_iterations=20)
    assert sorted(batch.out_lengths)[0] in shortest, batch.out_lengths
    sess.gradient()
    check_forward(LA, sess, batch, chain, seeds, 0, tag)
    sess.iterate(3)
    check_forward(LA, sess, batch, chain, seeds, 2, tag)
    sess.iterate(15)
    step = int(sess.step.cpu()[0])
    assert step == 18, step
    check_forward(LA, sess, batch, chain, seeds, 17, tag)
    return batch, seeds


def step_0_is_the_stand_alone_entry(rt, O, lengths, entry, alone):
    """Buffer 12 at step 0 of a session that holds [entry] (clips 30, 31, attack seeds 3, 4) is alone(x), the stand-alone entry
    on the same input, bit for bit.  The input x = N(N(y)) in the device's own rounding is buffer 12 of a second session whose
    entry never fires: the same buffer 9, and within 2e-7 of the float64 value."""
    clips = list(range(30, 30 + len(lengths)))
    on, batch, _, _ = session(rt, O, lengths, clips, [entry], [3, 4])
    off, _, _, _ = session(rt, O, lengths, clips, [dict(entry, prob=0.0)], [3, 4])
    on.gradient()
    off.gradient()
    torch.cuda.synchronize()
    assert torch.equal(on._view(9, (batch.total_out,)), off._view(9, (batch.total_out,))), "buffer 9 of the two sessions"
    x = rt.Ragged(off.attacked.clone(), batch.out_lengths)
    for b, (xi, y) in enumerate(zip(x.to_list(), synthesis(off, batch))):
        dx = float(np.abs(xi - norm2(y.double()).numpy()).max())
        assert dx < 2e-7, (b, dx)
    z = alone(x)
    assert torch.equal(z.data, on.attacked), float((z.data - on.attacked).abs().max())
    assert not torch.equal(z.data, x.data), "the entry left every clip as it was"


# ---- first gradient -------------------------------------------------------------------------------------------------------------------
def check_gradient(rt, O, LA, chain, lengths, clip_seed0, drawn, exercised, describe, **kw):
    """The pv rule.  aware_embed_gradient against autograd over the float64 restatement composed with the oracle's loop body.  The
    bound on the relative L2 distance of a clip's gradient is four times the distance of the same composition in float32 from it,
    computed here on the CPU, and at least the 2e-5 the older kinds hold.  Loss and prediction are held the same way: within four
    times the float32 composition's own distance from the float64 one, and at least the 1e-6 the older kinds hold.  The older
    kinds' 1e-6 alone is not a floor here: behind the vocoder's STFT the float32 torch restatement itself, with no device code
    involved, lands up to 8.9e-7 (prediction) and 2.4e-7 (loss) from the float64 one.  No clip closer than
    KINK to a LeakyReLU kink in either precision.

    drawn(LA, chain, seed, step, ny) is the module's draw of its entry, describe(draw) its words in the printed line, and
    exercised(draw, i, ny) says that clip i's draw puts the operator to work."""
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
        d = drawn(LA, chain, seeds[i], 0, batch.out_lengths[i])
        print(f"{kw} clip {i} (n = {lengths[i]}, {describe(d)}): loss err {lerr:.1e} (float32 restatement {lfloor:.1e}), pred err "
              f"{perr:.1e} ({pfloor:.1e}), gradient rel L2 {rel:.2e} ({floor:.2e}), nearest LeakyReLU kink {kink:.1e} / {kink32:.1e}")
        assert exercised(d, i, batch.out_lengths[i]), ("the case is to exercise the operator", i, d)
        assert min(kink, kink32) >= KINK, (i, kink, kink32)
        assert lerr <= max(4 * lfloor, 1e-6) and perr <= max(4 * pfloor, 1e-6), (i, lerr, lfloor, perr, pfloor)
        assert rel <= max(4 * floor, 2e-5), (i, rel, floor)


def first_gradient(rt, O, LA, chain, lengths, clip_seeds, band=(32, 256), **kw):
    """The figures of the older kinds' rule: aware_embed_gradient, loss and prediction at step 0 against autograd over the
    restatement composed with the oracle's loop body in the oracle's own float32.  Returns the batch, the attack seeds and per
    clip (relative L2 of the gradient, nearest LeakyReLU kink, loss error, prediction error); the caller prints and asserts."""
    from test_gpu_kernels import _min_kink_distance
    seeds = [5 + 2 * i for i in range(len(lengths))]
    sess, batch, pairs, wm = session(rt, O, lengths, clip_seeds, chain, seeds, band=band, use_graph=False, **kw)
    g = sess.gradient()
    torch.cuda.synchronize()
    g = g.cpu()
    loss, pred = sess.loss.cpu().numpy(), sess.pred.cpu().numpy()
    nb = band[1] - band[0] + 1
    figures = []
    for i, (clip, _) in enumerate(pairs):
        emb = attacked_oracle(O, LA, chain, seeds[i], 0, None if band == (32, 256) else band)
        mag0, phase = emb.analyse(torch.from_numpy(clip)[None])
        c0 = mag0[:, emb.band].clone().requires_grad_(True)
        l, p = emb.forward_loss(c0, mag0, phase, torch.from_numpy(wm[i])[None])
        l.sum().backward()
        ref = c0.grad[0]
        mine = g[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :nb].T
        rel = (mine - ref).norm().item() / ref.norm().item()
        lerr, perr = abs(loss[i] - float(l.detach())), float(np.abs(pred[i] - p[0].detach().numpy()).max())
        figures.append((rel, _min_kink_distance(emb, mag0, phase), lerr, perr))
    return batch, seeds, figures


def check_first_gradient(rt, O, LA, chain, lengths, band=(32, 256), **kw):
    """The rule of kinds 0, 1, 2 and 8 on clips 40, 41, ...: 2e-5 relative L2 per clip (2e-2 for a clip with a LeakyReLU argument
    within 2e-6 of its kink), loss and prediction 1e-5."""
    _, _, figures = first_gradient(rt, O, LA, chain, lengths, list(range(40, 40 + len(lengths))), band, **kw)
    for i, (rel, kink, lerr, perr) in enumerate(figures):
        print(f"{kw} band {band} clip {i} (n = {lengths[i]}): loss err {lerr:.1e}, pred err {perr:.1e}, "
              f"gradient rel L2 {rel:.2e}, nearest LeakyReLU kink {kink:.1e}")
        assert lerr < 1e-5 and perr < 1e-5, (i, lerr, perr)
        assert rel < (2e-5 if kink > 2e-6 else 2e-2), (i, rel, kink)


# ---- an entry that never fires, or not on every clip ------------------------------------------------------------------------------------
def prob_0_is_the_plain_loop(rt, O, chains, lengths=(8000, 16000, 24000)):
    """Each of `chains`, whose entries never fire, against the loop without a chain on clips 62, 63, 64: coefficients, best
    coefficients and losses after 20 steps and the gradient of step 20, bit for bit, on both dsp_paths, and buffer 12 within 2e-7
    of N(N(buffer 9))."""
    lengths = list(lengths)
    for dsp_path in ("stream", "staged"):
        plain, _, _, _ = session(rt, O, lengths, [62, 63, 64], None, num_iterations=21, dsp_path=dsp_path)
        plain.iterate(20)
        gp = plain.gradient()
        for chain in chains:
            att, batch, _, _ = session(rt, O, lengths, [62, 63, 64], chain, num_iterations=21, dsp_path=dsp_path)
            att.iterate(20)
            ga = att.gradient()
            torch.cuda.synchronize()
            for b, (z, y) in enumerate(zip(attacked(att, batch), synthesis(att, batch))):
                dz = float((z.double() - norm2(y.double())).abs().max())
                assert dz < 2e-7, (dsp_path, chain, b, dz)
            dc, dl = float((plain.coef - att.coef).abs().max()), float((plain.loss - att.loss).abs().max())
            print(f"{dsp_path}, prob 0 against the plain loop after 20 steps: max |coef difference| = {dc:.3e}, loss difference {dl:.3e}")
            assert torch.equal(plain.coef, att.coef) and torch.equal(plain.best_coef, att.best_coef), (dsp_path, chain, dc)
            assert torch.equal(plain.loss, att.loss) and torch.equal(plain.best_loss, att.best_loss), (dsp_path, chain, dl)
            assert torch.equal(gp, ga), (dsp_path, chain, float((gp - ga).abs().max()))


def does_not_fire_keeps_its_bits(rt, O, LA, entry, drawn, apply, fired):
    """`entry` with prob 0.5 on three clips, 8 steps: where it does not fire, buffer 12 is N(N(buffer 9)) in the device's rounding,
    bit for bit; where it fires, apply(x, z, draw) says that z is the operator's output for x.  fired(draw, ny) tells the two
    cases the module wants to see apart; both occur."""
    lengths, seeds = [16000, 8000, 24000], [1, 2, 3]
    chain = LA.parse_chain([dict(entry, prob=0.5)])
    sess, batch, _, _ = session(rt, O, lengths, [70, 71, 72], chain, seeds, num_iterations=20)
    seen = set()
    for step in range(8):
        sess.iterate(1)
        torch.cuda.synchronize()
        for b, (y, z) in enumerate(zip(synthesis(sess, batch), attacked(sess, batch))):
            d = drawn(LA, chain, seeds[b], step, len(y))
            x = device_x(y.numpy())
            if d[0]:
                assert apply(x, z.numpy(), d), (step, b, d)
            else:
                assert bits_equal(z.numpy(), x), (step, b, d)
            seen.add(fired(d, len(y)))
    assert seen == {False, True}, seen


# ---- graph replay ---------------------------------------------------------------------------------------------------------------------
def graph_replay_bits(rt, O, chain, lengths, first=32, more=()):
    """`first` + 8 steps on clips 50, 51, ... under graph replay and without it: the coefficients, the best coefficients, the best
    losses and, after each of the last 8 steps, the losses, buffer 12 and the session attributes `more` names, bit for bit.
    Returns the replayed run's tuple, in that order, and the batch, for the module's own check that the draws moved."""
    names = ("coef", "best_coef", "best_loss", "loss", "attacked") + tuple(more)
    out = []
    for use_graph in (True, False):
        sess, batch, _, _ = session(rt, O, lengths, list(range(50, 50 + len(lengths))), chain, num_iterations=first + 8, use_graph=use_graph)
        per_step = [[] for _ in range(2 + len(more))]
        sess.iterate(first)
        for _ in range(8):
            sess.iterate(1)
            for rec, name in zip(per_step, names[3:]):
                rec.append(getattr(sess, name).clone())
        torch.cuda.synchronize()
        out.append((sess.coef.cpu(), sess.best_coef.cpu(), sess.best_loss.cpu()) + tuple(torch.stack(rec).cpu() for rec in per_step))
        step = int(sess.step.cpu()[0])
        assert step == first + 8, (use_graph, step)
    for name, a, b in zip(names, *out):
        assert torch.equal(a, b), (name, float((a.double() - b.double()).abs().max()))
    return out[0], batch


# ---- a mixture --------------------------------------------------------------------------------------------------------------------------
def mixture_is_its_chains(rt, O, LA, chain, other, lengths=(16000, 8000, 16000, 8000), bound=None):
    """A mixture of `chain` and `other`, half each, at step 0: buffer 14 holds the host's choices, and every clip's buffer 12 (with
    buffer 9, loss, prediction and its rows of the coefficient gradient) is bit for bit that of a session that holds only the
    chain the clip drew.  With a `bound`, the clips that drew `chain` are within it of the float64 restatement's peak."""
    lengths = list(lengths)
    mixture = LA.parse_mixture([{"weight": 0.5, "chain": chain}, {"weight": 0.5, "chain": other}])
    s0 = 0
    while set(LA.mixture_choices(list(range(s0, s0 + 4)), 0, [0.5, 0.5]).tolist()) != {0, 1}:
        s0 += 1
    seeds = list(range(s0, s0 + 4))
    choice = LA.mixture_choices(seeds, 0, [0.5, 0.5])
    kw = dict(num_iterations=4)
    mix, batch = mixture_session(rt, O, lengths, seeds, mixture=mixture, **kw)
    g = mix.gradient()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(mix.choices.cpu().numpy(), choice)
    z, y, loss, pred = mix.attacked.clone(), mix._view(9, (batch.total_out,)).clone(), mix.loss.clone(), mix.pred.clone()
    for c in (0, 1):
        one, _ = mixture_session(rt, O, lengths, seeds, chain=mixture[c]["chain"], **kw)
        g1 = one.gradient()
        torch.cuda.synchronize()
        y1 = one._view(9, (batch.total_out,))
        for b in np.flatnonzero(choice == c):
            assert torch.equal(y[span(batch, b)], y1[span(batch, b)]) and torch.equal(z[span(batch, b)], one.attacked[span(batch, b)]), (b, c)
            assert torch.equal(loss[b], one.loss[b]) and torch.equal(pred[b], one.pred[b]), (b, c)
            assert torch.equal(g[rows(batch, b)], g1[rows(batch, b)]) and float(g[rows(batch, b)].abs().max()) > 0.0, (b, c)
    if bound is not None:
        for b in np.flatnonzero(choice == 0):
            yb, zb = y[span(batch, b)].cpu(), z[span(batch, b)].cpu()
            ref = LA.apply_chain(norm2(yb.double())[None], mixture[0]["chain"], [seeds[b]], 0)[0]
            err = float((zb.double() - ref).abs().max() / ref.abs().max())
            assert err < bound, (b, err, bound)


# ---- the other synthesis run lengths ------------------------------------------------------------------------------------------------------
def forward_at_run_length(rt, O, LA, bname, kind, chain, check_forward):
    """The batch `bname` of tests/test_gpu_loop_run_lengths.py (a synthesis run of 12, 8 or 6 hop blocks) with `chain` in the loop:
    buffer 12 of the five head clips at steps 0 and 2 by the module's own check_forward, and finite and not all zero."""
    from test_gpu_loop_run_lengths import COMPARED, big_session      # the batches live with the module that is about them
    sess, batch, seeds = big_session(rt, O, bname, kind, chain=chain, num_iterations=4)
    sess.gradient()
    check_forward(LA, sess, batch, chain, seeds, 0, f"{bname} {kind}", sample=COMPARED[bname])
    sess.iterate(3)
    step = int(sess.step.cpu()[0])
    assert step == 3, step
    check_forward(LA, sess, batch, chain, seeds, 2, f"{bname} {kind}", sample=COMPARED[bname])
    z = sess.attacked
    assert bool(torch.isfinite(z).all()) and float(z.abs().max()) > 0.0, (bname, kind, float(z.abs().max()))


# ---- workspace ----------------------------------------------------------------------------------------------------------------------------
def older_chains_workspace(rt, O):
    """On the batch [16000, 8000] the seven older chains need the bytes they needed, through the _ex entry and, for noise and
    suppression, through the older one.  Returns size(entries), the seven byte counts by name, and the batch."""
    sess, batch, _, _ = session(rt, O, RAGGED, [64, 65], None, num_iterations=20, use_graph=False)
    lib = sess.lib
    size = lambda ent: lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries(ent), len(ent))
    nb = {name: size(ent)
          for name, ent in (("noise", [NO]), ("noise_suppression", [NO, SU]), ("reverb", [RV]), ("suppression_reverb_noise", [SU, RV, NO]),
                            ("speed", [SP]), ("noise_speed", [NO, SP]), ("four", [NO, SU, SP, NO]))}
    print("workspace bytes:", nb)
    assert nb == PARENT_WORKSPACE, nb
    old = lib.aware_embed_loop_attack_workspace_bytes(batch.h, 2)
    assert old == PARENT_WORKSPACE["noise_suppression"], old
    return size, nb, batch


# ---- cards ----------------------------------------------------------------------------------------------------------------------------------
def card():
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        return yaml.safe_load(f)


def stereo_round_trip(tmp_path, card_yaml, entry):
    """load() of a card with `card_yaml` as its loop_attacks, which parses to [entry]; then embed_watermark / detect_watermark on
    a stereo clip: every channel carries the payload."""
    from aware_amd.embedding.loop_attacks import parse_chain
    from aware_amd.service import detect_watermark, embed_watermark
    from aware_amd.utils.models import load
    c = card()
    c["loop_attacks"] = yaml.safe_load(card_yaml)
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(c))
    emb, det = load(str(p))
    assert emb.loop_attacks == parse_chain([entry]), (emb.loop_attacks, entry)
    bits = np.random.default_rng(29).integers(0, 2, 20).astype(np.int32)
    stereo = np.column_stack([make_clip(51, 16000)[0], make_clip(52, 16000)[0]])
    out = embed_watermark(stereo, 16000, bits, emb)
    assert out.shape[1] == 2 and np.isfinite(out).all(), out.shape
    got = detect_watermark(out, 16000, det)
    for ch in (got if isinstance(got, (list, tuple)) else [got]):
        np.testing.assert_array_equal(np.asarray(ch).reshape(-1)[:20].astype(np.int32), bits)


def value_claim_setup(O, tmp_path):
    """The value claims' experiment: four 1 s clips, seeds 0..3, their payloads, and two functions.  embed(chain) loads the card
    with `chain` as its loop_attacks (None: the plain card), checks that it parsed, embeds the four clips in 400 steps and returns
    the waveforms as a list of arrays and the detector; ber(det, ys) is the bit error rate in % of a list, an array of rows or a
    Ragged."""
    from aware_amd.embedding.loop_attacks import parse_chain
    from aware_amd.utils.models import load
    base = card()
    pairs = [make_clip(s, 16000) for s in range(4)]
    clips, bits = [p[0] for p in pairs], np.stack([p[1] for p in pairs])
    wm = np.stack([O.bits_to_bipolar(b) for b in bits]).astype(np.float32)

    def embed(chain):
        c = dict(base)
        if chain:
            c["loop_attacks"] = chain
        p = tmp_path / "card.yaml"
        p.write_text(yaml.safe_dump(c))
        emb, det = load(str(p))
        assert emb.loop_attacks == parse_chain(chain), (emb.loop_attacks, chain)
        return [o.cpu().numpy() for o in emb.embed_batch(clips, 16000, wm)], det

    def ber(det, ys):
        vals = det.detect_batch(ys.to_list() if hasattr(ys, "to_list") else list(ys), 16000).cpu().numpy()
        return 100.0 * float((O.decode_bits(vals) != bits).mean())

    return clips, bits, embed, ber
