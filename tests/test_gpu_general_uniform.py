"""The general route (key general_geometry; DESIGN.md sections 31 and 33) on the batches embed_batch exists for, at every
optimiser step, and at its output, against GeneralLoop(..., dtype=torch.float64) of tests/test_general_geometry_host.py.

A. Uniform batches.  tests/test_gpu_general_geometry.py runs ragged batches of four clips, for which det_plan (csrc/capi.hip)
   chooses the ragged conv kernels, the mel GEMM with mel_norm and the three-kernel read-out.  The cases UA to UF of
   tests/test_general_uniform_host.py (its docstring has the table) are many clips of one length: det_plan gives them the
   clip-aligned conv kinds (ClipH2 on "f16x2", ClipX3 on "bf16x3", ClipF32 on "f32"), the fused read-out, and from 192 clips
   on mel_front_x3_kernel and mel_back_x3_kernel, which walk K = lda = the band stride: 64, 128, 192 and 2112 floats here,
   never the card's 256; UE has 16 frames and 8 pooled rows per clip.  Compared are slots 0, 1, B/2 - 1, B/2, B - 2 and B - 1,
   whose clips keep clear of every LeakyReLU kink (checked on the CPU by the host module), so no bound has a kink exception.
   Forms reported by conv_tiles() under conv_tile="auto" on "f16x2", (forward, backward) per conv block (128 -> 512 -> 1024 ->
   1024 -> 40 channels), 2 = wide, 1 = narrow, 0 = no f16 two-term launch (the last block belongs to the fused read-out, block
   0's data gradient to the mel backward): ([1, 2, 2, 0], [0, 1, 2, 0]) for UA to UE (a 1024-channel GEMM fills 768 or 772
   workgroups of the wide form, above kH2WideMinGrid = 512; a 512-channel one 384 or 386) and ([1, 1, 1, 0], [0, 1, 1, 0]) for
   UF; ([2, 2, 2, 0], [0, 2, 2, 0]) under "wide" and ([1, 1, 1, 0], [0, 1, 1, 0]) under "narrow" in every case.
B. Every step.  lr = 3.0 makes clips fail to improve at some steps (at the card's 0.1 every clip improves at almost every
   step, so neither a wrong clip index in band_coef_grad_kernel<true> nor a best snapshot that always copies would change
   anything another test looks at).  Every step of the fused NAdam kernel is replayed on the host in float64 from the session's
   own gradient, and the best snapshot from the session's own losses; the same for Adam under cosine annealing, which steps
   in launch_opt_rows.
C. The output.  aware_embed_finish (band_assemble, gen_synthesis, rescale_normalize_kernel) against the float64 restatement
   fed the device's best coefficients, and with a signed rescale.
D. Graph replay against plain launches, bit for bit.

Run on the MI355X box:  python -m pytest tests/test_gpu_general_uniform.py -m gpu -q -s
"""
import copy

import numpy as np
import pytest
import torch

from conftest import make_clip
from oracle import aware_oracle as O
from test_general_uniform_host import (CASES, REGISTRY, STEP_COUNT, STEP_LR, check_non_improvement, compared_slots,
                                       general_loop, slot_seeds)
from test_gpu_general_geometry import STRIDE, case, trivial
from test_gpu_mel_norm_bits import constant, entry_plan_args, mel_kinds
from test_gpu_registry import STEP_BOUND, STEP_BOUND_CAP, host_schedulers

pytestmark = pytest.mark.gpu

RUNS = [(name, pipe) for name in CASES for pipe in ("bf16x3", "f16x2")] + [("UC", "f32")]
GRAD_BOUND = {"bf16x3": 2e-4, "f16x2": 2e-3, "f32": 2e-4}     # test_first_step's; "f32" (full-precision MFMA) takes the tighter one


@pytest.fixture(scope="module")
def rt():
    from aware_amd import runtime
    from aware_amd._lib import require_gpu
    require_gpu()
    return runtime


# ---- the batches and their references: built once, shared, never modified ------------------------------------------------------
_UCASES, _REFS, _FIRST = {}, {}, {}


def ucase(rt, name):
    """Plan, detector and embedder of the case's geometry (test_gpu_general_geometry.case), its batch, packed audio, payloads."""
    if name not in _UCASES:
        geom, n, B, _ = CASES[name]
        c = case(rt, geom)
        seeds = slot_seeds(name)
        pairs = {s: make_clip(s, n) for s in set(seeds)}
        clips = [pairs[s][0] for s in seeds]
        wm = np.stack([(2 * pairs[s][1] - 1).astype(np.float32) for s in seeds])
        batch = c["emb"].make_batch([n] * B, c["sr"])
        assert batch.B == B and len(set(batch.frames)) == 1 and batch.in_offsets == [n * i for i in range(B)]
        _UCASES[name] = dict(geom=geom, n=n, B=B, plan=c["plan"], dev=c["dev"], det=c["det"], sr=c["sr"], batch=batch, clips=clips,
                             wm=wm, audio=torch.from_numpy(np.concatenate(clips)).cuda(), target=torch.from_numpy(wm).cuda(),
                             slots=compared_slots(B), seeds=seeds)
    return _UCASES[name]


def reference(u, i):
    """float64 restatement of slot i's clip: detect values, and loss, prediction and gradient [T, nband] of the first loop body."""
    key = (u["geom"], u["n"], u["seeds"][i])
    if key not in _REFS:
        e64 = general_loop(u["geom"])
        x = torch.from_numpy(u["clips"][i]).double()[None]
        loss, pred, g = e64.first_iteration(x, torch.from_numpy(u["wm"][i]).double()[None])
        _REFS[key] = dict(vals=e64.detect_raw(x)[0].numpy(), loss=float(loss[0]), pred=pred[0].numpy(), grad=g[0].T.contiguous())
    return _REFS[key]


def rows(batch, i):
    return slice(batch.frame_offsets[i], batch.frame_offsets[i + 1])


def first_step(rt, name, pipe, tile="auto"):
    """Loss, prediction, gradient and conv_tiles() of a session's first loop body on the case's batch."""
    if (name, pipe, tile) not in _FIRST:
        u = ucase(rt, name)
        sess = rt.EmbedSession(u["plan"], u["dev"], u["batch"], use_graph=False, conv_pipe=pipe, conv_tile=tile)
        sess.begin(u["audio"], u["target"])
        g = sess.gradient()
        torch.cuda.synchronize()
        _FIRST[name, pipe, tile] = dict(g=g.cpu(), loss=sess.loss.cpu().clone(), pred=sess.pred.cpu().clone(), tiles=sess.conv_tiles())
    return _FIRST[name, pipe, tile]


# ---- A. uniform batches -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pipe", RUNS, ids=[f"{n}-{p}" for n, p in RUNS])
def test_the_batch_takes_the_kernels_it_is_meant_for(rt, name, pipe):
    """det_plan's rules restated (mel_kinds of tests/test_gpu_mel_norm_bits.py, kMelFrontMinClips read from the source):
    mel_front_x3_kernel and mel_back_x3_kernel for UA to UE on the MFMA pipes that have them, the mel GEMM for UF and for
    "f32"; aware_detect takes the front kernel for the same cases.  On "f16x2" every conv block with 128 or more output
    channels reports a form of the f16 two-term kernel, the data gradients of blocks 1 and 2 too, and the chip-filling cases
    take the wide form for the 1024-channel GEMMs without being forced (h2_conv_tile)."""
    u = ucase(rt, name)
    geom, _, B, (T, pooled, groups) = CASES[name]
    batch, dev = u["batch"], u["dev"]
    assert batch.frames == [T] * B and batch.total_pooled >= pooled * B and u["plan"].band_stride == STRIDE[geom]
    ch = rt.stored_channels(case(rt, geom)["emb"].detection_net.channels)
    assert ch == list(dev.channels) and dev.is_card
    min_clips = constant("capi.hip", "kMelFrontMinClips")
    kinds = mel_kinds(ch, u["plan"].band_stride, dev.is_card, batch.frames, rt.CONV_PIPES[pipe], False, min_clips)
    assert kinds == ((True, True) if name != "UF" and pipe != "f32" else (False, False)), (name, pipe, kinds)
    det_pipe, _, det_training = entry_plan_args("aware_detect")
    assert mel_kinds(ch, u["plan"].band_stride, dev.is_card, batch.frames, det_pipe, det_training, min_clips)[0] == (name != "UF")
    fwd, bwd = first_step(rt, name, pipe)["tiles"]
    print(f"{name} {pipe}: {B} clips of {T} frames ({groups} row groups), rows of {STRIDE[geom]} floats: mel front / back {kinds}, "
          f"conv_tiles under auto {fwd} / {bwd}")
    if pipe != "f16x2":
        assert not any(fwd) and not any(bwd)
        return
    assert all(fwd[l] != 0 for l in range(len(fwd)) if ch[l + 1] >= 128), (name, fwd)
    assert all(bwd[l] != 0 for l in range(1, len(bwd) - 1)), (name, bwd)      # data gradients of 512 and 1024 channels
    assert (2 in fwd) == (name != "UF"), (name, fwd)                 # at least one case is wide under "auto"; here: five


@pytest.mark.parametrize("name,pipe", RUNS, ids=[f"{n}-{p}" for n, p in RUNS])
def test_first_step(rt, name, pipe):
    """sess.loss and aware_embed_gradient of the compared slots against first_iteration in float64, by test_first_step's
    bounds: loss 5e-5 * max(1, |loss|), gradient relative L2 2e-4 on bf16x3 (and on f32) and 2e-3 on f16x2; the padding
    columns [nband, stride) of every gradient row are exactly 0."""
    u = ucase(rt, name)
    mine = first_step(rt, name, pipe)
    g, loss = mine["g"].double(), mine["loss"].numpy()
    nb, batch = u["plan"].nband, u["batch"]
    assert torch.isfinite(g).all() and np.isfinite(loss).all()
    assert g.shape[1] == STRIDE[u["geom"]] > nb and float(g[:, nb:].abs().max()) == 0.0
    figures = []
    for i in u["slots"]:
        r = reference(u, i)
        el = abs(float(loss[i]) - r["loss"]) / max(1.0, abs(r["loss"]))
        rel = float((g[rows(batch, i), :nb] - r["grad"]).norm() / r["grad"].norm())
        figures.append((i, el, rel))
        print(f"{name} {pipe} slot {i}: loss err {el:.1e} (bound 5e-5), gradient rel L2 {rel:.2e} (bound {GRAD_BOUND[pipe]:.0e})")
    for i, el, rel in figures:
        assert el < 5e-5, (name, pipe, i, el)
        assert rel < GRAD_BOUND[pipe], (name, pipe, i, rel)


@pytest.mark.parametrize("name", list(CASES))
def test_detect(rt, name):
    """det.detect_batch on the same batch, compared slots against detect_raw in float64: 1e-4, as test_detect."""
    u = ucase(rt, name)
    vals = u["det"].detect_batch(u["clips"], u["sr"]).cpu().numpy()
    assert vals.shape == (u["B"], 20) and np.isfinite(vals).all()
    err = [float(np.max(np.abs(vals[i] - reference(u, i)["vals"]))) for i in u["slots"]]
    print(f"{name}: max |detect - float64 restatement| at slots {u['slots']}: {['%.1e' % e for e in err]} (bound 1e-4)")
    assert max(err) < 1e-4, (name, err)
    assert np.array_equal(vals[u["B"] - 1], vals[0])


@pytest.mark.parametrize("name,pipe", RUNS, ids=[f"{n}-{p}" for n, p in RUNS])
def test_no_cross_talk(rt, name, pipe):
    """Slot B - 1 holds slot 0's clip and payload: its loss, prediction and gradient rows are slot 0's bit for bit, and no
    other compared slot's."""
    u = ucase(rt, name)
    mine, batch, last = first_step(rt, name, pipe), u["batch"], u["B"] - 1
    assert torch.equal(mine["loss"][last], mine["loss"][0]) and torch.equal(mine["pred"][last], mine["pred"][0])
    assert torch.equal(mine["g"][rows(batch, last)], mine["g"][rows(batch, 0)])
    for i in u["slots"][1:-1]:
        assert not torch.equal(mine["g"][rows(batch, i)], mine["g"][rows(batch, 0)]), (name, pipe, i)


@pytest.mark.parametrize("name", list(CASES))
def test_tile_forms_give_the_same_bits(rt, name):
    """EmbedSession's docstring: the 128-column form and the wide form of the f16 two-term conv kernel give the same bits.
    Every case has at most three row groups per clip and blocks of 512 and 1024 channels, so the library accepts "wide" in all
    of them (a refusal raises): loss, prediction and gradient under "narrow", "wide" and "auto", bit for bit."""
    assert CASES[name][3][2] <= 3
    narrow, wide, auto = (first_step(rt, name, "f16x2", t) for t in ("narrow", "wide", "auto"))
    print(f"{name}: conv_tiles narrow {narrow['tiles']}, wide {wide['tiles']}, auto {auto['tiles']}")
    assert set(narrow["tiles"][0] + narrow["tiles"][1]) == {0, 1} and 2 in wide["tiles"][0] and 2 in wide["tiles"][1]
    for other in (wide, auto):
        assert torch.equal(narrow["g"], other["g"]) and torch.equal(narrow["loss"], other["loss"])
        assert torch.equal(narrow["pred"], other["pred"])


# ---- B. every step, with steps that do not improve ------------------------------------------------------------------------------
STEP_BATCHES = ["G2-ragged", "UA"]
_DONE = {}


def step_batch(rt, which):
    """(plan, detector weights, batch, packed audio, payloads on the device, clips, compared clips, clips with one pooled frame)."""
    if which == "UA":
        u = ucase(rt, "UA")
        return u["plan"], u["dev"], u["batch"], u["audio"], u["target"], u["clips"], u["slots"], [], "G1"
    c = case(rt, "G2")
    short = [i for i in range(len(c["lengths"])) if trivial("G2", i)]
    assert len(short) == 1
    return (c["plan"], c["dev"], c["batch"], c["batch"].pack(c["clips"]), torch.from_numpy(c["wm"]).cuda(), c["clips"],
            list(range(len(c["lengths"]))), short, "G2")


def check_begin(sess, batch, nb, geom, clips, compared):
    """The state aware_embed_begin leaves: coef against the float64 band magnitude (1e-5 of the clip's largest), lo and hi
    within 2 ulp of the box of the device's own coef with lo >= 0 (the bound of test_bounds_vs_oracle_and_golden), zero
    padding, best_coef == coef and best_loss == inf."""
    coef, best = sess.coef.cpu().clone(), sess.best_coef.cpu().clone()
    lo, hi = (t.cpu().clone() for t in sess.bounds)
    for t in (coef, lo, hi, best):
        assert float(t[:, nb:].abs().max()) == 0.0
    assert torch.equal(coef, best) and bool(torch.isinf(sess.best_loss.cpu()).all()) and bool((sess.best_loss.cpu() > 0).all())
    assert bool((lo >= 0).all()) and bool((lo <= hi).all())
    e64, e32 = general_loop(geom), O.Embedder()
    worst = 0.0
    for i in range(batch.B):
        c = coef[rows(batch, i), :nb]
        scale = float(c.max())
        l2, h2 = e32.bounds(c)
        ulp = float(np.spacing(np.float32(scale)))
        assert float((lo[rows(batch, i), :nb] - l2).abs().max()) <= 2 * ulp, i
        assert float((hi[rows(batch, i), :nb] - h2).abs().max()) <= 2 * ulp, i
        if i in compared:
            mag0, _ = e64.analyse(torch.from_numpy(clips[i]).double()[None])
            cref = mag0[0, e64.band].T
            err = float((c.double() - cref).abs().max()) / float(cref.max())
            worst = max(worst, err)
            assert err < 1e-5, (i, err)
    return coef, worst


def replay_best(best, best_loss, loss, got, batch):
    """The reference's rule (multibit_embedder.py:120-122): a clip whose pre-step loss is below its best so far snapshots
    its post-step coefficients.  In place; from the device's own losses, strict <."""
    for i in range(batch.B):
        if loss[i] < best_loss[i]:
            best_loss[i] = loss[i]
            best[rows(batch, i)] = got[rows(batch, i)]


@pytest.mark.parametrize("which", STEP_BATCHES)
def test_every_fused_nadam_step(rt, which):
    """Ten steps of band_coef_grad_kernel<true> at lr = 3.0: each against O.nadam_step with O.nadam_schedule(10, lr=3.0) and
    the clamp, in float64, applied to the device's previous coefficients and the gradient the session reports at the same
    point: |got - p| / (1e-3 + |p|) < 2e-4 on the band and exactly 0 on the padding (the host replay and the bound of
    tests/test_gpu_wide_band.py::test_fused_nadam_steps_over_the_wide_row); best_coef bit for bit and best_loss exactly what
    the device's own losses make them.  The device's trajectory has steps at which one clip improves and another does not
    (asserted), so a wrong clip index or an unconditional snapshot fails here.  The clip with one pooled frame improves at
    step 0 only and its rows never move."""
    plan, dev, batch, audio, target, clips, compared, short, geom = step_batch(rt, which)
    nb, n = plan.nband, STEP_COUNT
    sess = rt.EmbedSession(plan, dev, batch, lr=STEP_LR, num_iterations=n, use_graph=False)
    sess.begin(audio, target)
    coef0, worst0 = check_begin(sess, batch, nb, geom, clips, compared)
    print(f"{which}: max |coef - float64 band magnitude| / clip maximum before the first step {worst0:.1e} (bound 1e-5)")
    cg, cm, bc2 = O.nadam_schedule(n, lr=STEP_LR)
    c0 = coef0.double()
    lo, hi = (c0 * (1 - 10 ** (-6.0 / 20))).clamp_min(0), c0 * (1 + 10 ** (-6.0 / 20))
    p = c0.clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    best, best_loss = coef0.clone(), np.full(batch.B, np.inf, dtype=np.float32)
    traj, worst = [], 0.0
    for it in range(n):
        g = sess.gradient().cpu()
        loss = sess.loss.cpu().numpy().copy()
        traj.append(loss)
        sess.iterate(1)
        got = sess.coef.cpu().clone()
        O.nadam_step(p, g.double(), m, v, cg[it], cm[it], bc2[it])
        p = torch.minimum(torch.maximum(p, lo), hi)
        err = float(((got.double() - p).abs() / (1e-3 + p.abs()))[:, :nb].max())
        worst = max(worst, err)
        assert err < 2e-4, (which, it, err)
        assert float(got[:, nb:].abs().max()) == 0.0
        replay_best(best, best_loss, loss, got, batch)
        assert torch.equal(sess.best_coef.cpu(), best), (which, it)
        assert np.array_equal(sess.best_loss.cpu().numpy(), best_loss), (which, it)
        for i in short:
            assert float(g[rows(batch, i)].abs().max()) == 0.0 and abs(float(loss[i]) - 1.0) < 5e-5
            assert torch.equal(got[rows(batch, i)], coef0[rows(batch, i)]) and torch.equal(best[rows(batch, i)], coef0[rows(batch, i)])
        p = got.double()               # the next step starts where the kernel left off (moments carried on the host)
    traj = np.stack(traj)
    imp = check_non_improvement(traj, which)
    moving = [i for i in range(batch.B) if i not in short]
    mixed = [s for s in range(1, n) if imp[s, moving].any() and not imp[s, moving].all()]
    print(f"{which}: max step error {worst:.2e} (bound 2e-4); (clip, step) pairs without improvement {int((~imp).sum())} of "
          f"{imp.size}, steps at which some moving clips improve and others do not {mixed}")
    for i in compared[:4]:
        print(f"    clip {i}: losses {[round(float(x), 4) for x in traj[:, i]]}, no improvement at steps {np.flatnonzero(~imp[:, i]).tolist()}")
    assert mixed and int((~imp[:, moving]).sum()) >= 3
    for i in short:
        assert imp[:, i].tolist() == [True] + [False] * (n - 1)
    _DONE[which] = sess


def test_every_registry_step(rt):
    """Adam at lr = 0.5 under cosine_annealing on the ragged G2 batch (T_max = 3 over ten steps: the rate falls to 0 at step 3,
    where the step moves nothing and the loss repeats, and comes back; with T_max = 10 the restatement has one step without
    improvement in all, tests/test_general_uniform_host.py has the figures): the separate launch_opt_rows step and its
    own best snapshot, replayed as tests/test_gpu_registry.py (check_session_steps) replays the card route: one float64
    torch.optim step per clip from the device's coefficients on the gradient the session reports, at torch's own scheduler's
    rate, clamped to the box of c0; bound 3e-6 on |got - want| / (1e-3 + |want|) plus what an unrepeatable gradient() accounts
    for, never above 2e-4; the table's rate is torch's; best_coef bit for bit, best_loss exactly, zero padding, the step
    counter; and the same non-improvement condition from the device's own losses.  (check_session_steps itself requires every
    step to move the median element by 1e-3, which the step at rate 0 does not, so the replay is restated here; 25 % of the
    elements end on the box.)"""
    from aware_amd.embedding.optimizers import get_optimizer
    from aware_amd.embedding.schedulers import get_scheduler
    plan, dev, batch, audio, target, clips, compared, short, geom = step_batch(rt, "G2-ragged")
    nb, n, B = plan.nband, STEP_COUNT, batch.B
    name, params, sched, sparams = REGISTRY
    sess = rt.EmbedSession(plan, dev, batch, num_iterations=n, use_graph=False)
    opt = get_optimizer(name, None, **params)
    sess.set_optimizer(opt, get_scheduler(sched, opt, n, **sparams))
    sess.begin(audio, target)
    coef0, _ = check_begin(sess, batch, nb, geom, clips, compared)
    c0 = coef0.double()
    lo, hi = (c0 * (1 - 10 ** (-6.0 / 20))).clamp_min(0), c0 * (1 + 10 ** (-6.0 / 20))
    P = [c0[rows(batch, i), :nb].clone().requires_grad_(True) for i in range(B)]
    opts, scheds = host_schedulers(name, params, sched, sparams, P)
    best, best_loss = coef0.clone(), np.full(B, np.inf, dtype=np.float32)
    traj, worst, spread = [], 0.0, 0.0
    for it in range(n):
        pre = sess.coef.cpu().clone()
        g, g2 = sess.gradient().cpu(), sess.gradient().cpu()
        loss = sess.loss.cpu().numpy().copy()
        traj.append(loss)
        sess.iterate(1)
        assert int(sess.step.cpu()[0]) == it + 1
        got = sess.coef.cpu().clone()
        want, allowance = pre.double(), 0.0
        for i in range(B):
            r = rows(batch, i)
            np.testing.assert_allclose(sess._opt_table[it, 3], opts[i].param_groups[0]["lr"], rtol=1e-12)
            results = []
            for grad in ([g] if torch.equal(g, g2) else [g, g2]):
                o = opts[i] if grad is g else copy.deepcopy(opts[i])
                q = o.param_groups[0]["params"][0]
                with torch.no_grad():
                    q.copy_(pre[r, :nb].double())
                q.grad = grad[r, :nb].double()
                o.step()
                results.append(torch.minimum(torch.maximum(q.detach(), lo[r, :nb]), hi[r, :nb]).clone())
            want[r, :nb] = results[0]
            if len(results) > 1:
                allowance = max(allowance, float(((results[0] - results[1]).abs() / (1e-3 + results[0].abs())).max()))
            scheds[i].step()
        spread = max(spread, allowance)
        bound = STEP_BOUND + allowance
        assert bound <= STEP_BOUND_CAP, (it, allowance)
        err = float(((got.double() - want).abs() / (1e-3 + want.abs()))[:, :nb].max())
        worst = max(worst, err)
        assert err < bound, (it, err, bound)
        assert float(got[:, nb:].abs().max()) == 0.0
        replay_best(best, best_loss, loss, got, batch)
        assert torch.equal(sess.best_coef.cpu(), best), it
        assert np.array_equal(sess.best_loss.cpu().numpy(), best_loss), it
        for i in short:
            assert torch.equal(got[rows(batch, i)], coef0[rows(batch, i)]) and torch.equal(best[rows(batch, i)], coef0[rows(batch, i)])
    traj = np.stack(traj)
    imp = check_non_improvement(traj, "Adam, cosine annealing")
    moving = [i for i in range(B) if i not in short]
    dlo, dhi = (t.cpu() for t in sess.bounds)
    on_box = float(((got <= dlo) | (got >= dhi))[:, :nb].double().mean())
    print(f"Adam 0.5 / cosine on the ragged G2 batch: max step error {worst:.2e} (bound {STEP_BOUND:.0e} + gradient spread "
          f"{spread:.1e}); {100 * on_box:.0f} % of the elements on the box after {n} steps")
    for i in range(B):
        print(f"    clip {i}: losses {[round(float(x), 4) for x in traj[:, i]]}, no improvement at steps {np.flatnonzero(~imp[:, i]).tolist()}")
    assert [s for s in range(1, n) if imp[s, moving].any() and not imp[s, moving].all()]
    assert int((~imp[:, moving]).sum()) >= 3
    for i in short:
        assert imp[:, i].tolist() == [True] + [False] * (n - 1)


# ---- C. the output ------------------------------------------------------------------------------------------------------------
def stepped(rt, which):
    """The session test_every_fused_nadam_step left after its ten steps (or, run alone, one stepped here)."""
    if which not in _DONE:
        plan, dev, batch, audio, target, *_ = step_batch(rt, which)
        sess = rt.EmbedSession(plan, dev, batch, lr=STEP_LR, num_iterations=STEP_COUNT, use_graph=False)
        sess.begin(audio, target)
        sess.iterate(STEP_COUNT)
        _DONE[which] = sess
    return _DONE[which]


def synthesis(loop, clip, best):
    """GeneralLoop.embed's last lines in the loop's precision: the clip's analysis with the band replaced by `best`
    [nband, T], through istft and one normaliser."""
    with torch.no_grad():
        mag0, phase = loop.analyse(torch.from_numpy(clip).to(loop.dtype)[None])
        mag = mag0.clone()
        mag[:, loop.band] = best.to(loop.dtype)[None]
        y = loop.istft(mag * torch.exp(1j * phase))
        return (y / torch.amax(torch.abs(y) + 1e-8, dim=-1, keepdim=True))[0].double()


@pytest.mark.parametrize("which", STEP_BATCHES)
def test_finish_against_the_restatement(rt, which):
    """finish(None) after the ten steps, per compared clip, against the float64 restatement of the output fed the device's
    best_coef (float64 analysis of the clip, the band replaced, istft, one normaliser).  Bound: the larger of 2e-6 and four
    times the float32 restatement's distance from the float64 one on the same clip and coefficients, the rule
    tests/test_gpu_stft_general.py::test_geometry_grid_ragged has for aware_istft (the float32 restatement analyses the clip
    in float32 as the device does: both stand the same float32 spectrum next to the float64 one)."""
    plan, dev, batch, audio, target, clips, compared, short, geom = step_batch(rt, which)
    sess = stepped(rt, which)
    y = sess.finish(None).cpu().double()
    best = sess.best_coef.cpu()
    assert bool(torch.isfinite(y).all()) and not torch.equal(best, sess.coef.cpu())     # some clip kept an earlier step
    e64, e32 = general_loop(geom), general_loop(geom, torch.float32)
    figures = []
    for i in compared:
        b = best[rows(batch, i), :plan.nband].T
        mine = y[batch.out_offsets[i]: batch.out_offsets[i] + batch.out_lengths[i]]
        ref, r32 = synthesis(e64, clips[i], b.double()), synthesis(e32, clips[i], b)
        assert mine.shape == ref.shape
        err, floor = float((mine - ref).abs().max()), float((r32 - ref).abs().max())
        figures.append((i, err, floor))
        print(f"{which} clip {i}: max |finish - float64 restatement| {err:.2e}, float32 restatement {floor:.2e} "
              f"(bound {max(2e-6, 4 * floor):.2e}), peak {float(mine.abs().max()):.7f}")
    for i, err, floor in figures:
        assert err <= max(2e-6, 4 * floor), (which, i, err, floor)


@pytest.mark.parametrize("which", STEP_BATCHES)
def test_finish_with_a_signed_rescale(rt, which):
    """finish(rescale) is rescale[b] * finish(None) in float32, bit for bit (rescale_normalize_kernel computes r * (x / m)):
    one negative value (the service passes a signed maximum), 1.0, and values in (0, 1)."""
    plan, dev, batch, *_ = step_batch(rt, which)
    sess = stepped(rt, which)
    y = sess.finish(None)
    r = np.random.default_rng(7).uniform(0.05, 0.95, batch.B).astype(np.float32)
    r[:4] = [-0.75, 1.0, 0.5, 0.3]
    assert int((r < 0).sum()) == 1 and int((r == 1).sum()) == 1 and int(((r > 0) & (r < 1)).sum()) >= 2
    scaled = sess.finish(torch.from_numpy(r).cuda())
    per_sample = torch.repeat_interleave(torch.from_numpy(r), torch.tensor(batch.out_lengths)).cuda()
    assert batch.out_offsets == np.concatenate([[0], np.cumsum(batch.out_lengths)[:-1]]).tolist()
    want = per_sample * y
    d = (scaled - want).abs()
    print(f"{which}: finish(rescale) against rescale * finish(None): {int((scaled != want).sum())} of {want.numel()} samples differ, "
          f"max {float(d.max()):.1e}; clip 0 has peak {float(scaled[:batch.out_lengths[0]].abs().max()):.7f} and sign "
          f"{'flipped' if float((scaled[:batch.out_lengths[0]] * y[:batch.out_lengths[0]]).sum()) < 0 else 'kept'}")
    assert torch.equal(scaled, want)
    assert float((scaled[:batch.out_lengths[0]] * y[:batch.out_lengths[0]]).sum()) < 0
    assert torch.equal(sess.finish(None), y)


# ---- D. graph replay ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["UC", "G2-ragged"])
def test_graph_replay_is_bit_identical(rt, which):
    """Ten steps at lr = 3.0 with graph-captured steps and with plain launches: the loss per step, coef, best_coef, best_loss
    and finish(None) are equal bit for bit."""
    if which == "UC":
        u = ucase(rt, "UC")
        plan, dev, batch, audio, target = u["plan"], u["dev"], u["batch"], u["audio"], u["target"]
    else:
        plan, dev, batch, audio, target, *_ = step_batch(rt, which)
    out = []
    for use_graph in (True, False):
        sess = rt.EmbedSession(plan, dev, batch, lr=STEP_LR, num_iterations=STEP_COUNT, use_graph=use_graph)
        sess.begin(audio, target)
        losses = []
        for _ in range(STEP_COUNT):
            sess.iterate(1)
            losses.append(sess.loss.clone())
        torch.cuda.synchronize()
        assert int(sess.step.cpu()[0]) == STEP_COUNT
        out.append((torch.stack(losses), sess.coef.clone(), sess.best_coef.clone(), sess.best_loss.clone(), sess.finish(None)))
    imp = check_non_improvement(out[0][0].cpu().numpy(), which)
    print(f"{which}: graph replay against plain launches over {STEP_COUNT} steps; {int((~imp).sum())} (clip, step) pairs without improvement")
    for what, a, b in zip(("loss per step", "coef", "best_coef", "best_loss", "finish"), *out):
        assert torch.equal(a, b), (which, what, float((a - b).abs().max()))
