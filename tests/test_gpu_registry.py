"""The reference's third seam on the device: optimiser / scheduler registries (embedding/optimizers.py:3-20,
schedulers.py:3-16) -- element-wise updates against torch.optim on the CPU (what the reference runs), the session's separate
optimiser step (opt_rows_kernel) step by step against float64 torch.optim, its graph replay and reset, the per-clip
ReduceLROnPlateau state (plateau_kernel) against torch's, and embed sessions against the oracle's registry loop.

The case matrix, the input recipe and the float64 reference are those of tests/test_registry_host.py (which runs a float32
restatement of the kernels over them without a GPU)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import make_clip
from test_registry_host import (OPTIONS, TORCH_OPT, TORCH_SCHED, SCH, case_id, make_inputs, scheduler_params, seam_cases,
                                torch_reference)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from aware_amd import runtime
    from aware_amd._lib import require_gpu
    require_gpu()
    return runtime


CASES = [
    ("nadam", {"lr": 0.1}, None, None),
    ("nadam", {"lr": 0.05, "weight_decay": 0.01, "momentum_decay": 0.01}, "step", {"step_size": 5, "gamma": 0.7}),
    ("adam", {"lr": 0.02}, None, None),
    ("adam", {"lr": 0.02, "betas": (0.8, 0.99), "weight_decay": 0.05, "eps": 1e-6}, "cosine_annealing", {"T_max": 12, "eta_min": 1e-4}),
    ("adamw", {"lr": 0.03, "weight_decay": 0.1}, "exponential", {"gamma": 0.95}),
    ("sgd", {"lr": 0.05}, None, None),
    ("sgd", {"lr": 0.05, "momentum": 0.9, "nesterov": True, "weight_decay": 0.01}, "multi_step", {"milestones": [4, 11], "gamma": 0.5}),
    ("sgd", {"lr": 0.05, "momentum": 0.7, "dampening": 0.2}, "cyclic", {"base_lr": 0.01, "max_lr": 0.08, "step_size_up": 4}),
    ("rmsprop", {"lr": 0.01, "alpha": 0.95}, "cosine_annealing_warm_restarts", {"T_0": 6, "T_mult": 2}),
    ("adagrad", {"lr": 0.1, "lr_decay": 0.05}, None, None),
    ("adamax", {"lr": 0.02}, "cyclic", {"base_lr": 0.005, "max_lr": 0.05, "step_size_up": 3, "step_size_down": 5}),
    ("adadelta", {"lr": 1.0, "rho": 0.85}, None, None),
]
ON_BOX_CAP = 0.3            # share of elements on the box at the end (float64 reference): above it the clamp could hide an error
CLAMP_EXERCISED = {"nadam0-none-5000", "rmsprop0-cyclic-5000"}        # the float64 reference alone ends with 18 % / 22 % on the box


def _seam(rt, name, params, sched, sparams, n, steps, bounds="both", grad_scale=None, on_box_over=None):
    """`steps` carried steps of aware_opt_clamp_step (update + clamp, ONE kernel per step) against float64 torch.optim +
    torch.clamp with the same gradients.  bounds: which sides of the box exist ("both", "lo", "hi", "none"); grad_scale: the
    gradient-scale slot h8[7] (torch is fed grad * scale).  Relative error < 3e-6 over all elements and, separately, over
    the elements strictly inside the box; at most ON_BOX_CAP of the elements on the box at the end."""
    from aware_amd.embedding.optimizers import step_scalars
    p0, lo, hi, grads = make_inputs(name, n, steps)
    lo = lo if bounds in ("both", "lo") else None
    hi = hi if bounds in ("both", "hi") else None
    want = torch_reference(name, params, sched, sparams, p0, grads, lo, hi, grad_scale or 1.0)
    lo64 = np.full(n, -np.inf) if lo is None else lo.double().numpy()
    hi64 = np.full(n, np.inf) if hi is None else hi.double().numpy()
    mine = p0.clone().cuda()
    oc = rt.OptClamp(mine, name, steps, sched, sparams, **params)
    dlo, dhi = (None if lo is None else lo.cuda()), (None if hi is None else hi.cuda())
    worst = inner = 0.0
    for i in range(steps):
        g = grads[i].cuda()
        if grad_scale is None:
            oc.step(g, dlo, dhi)
        else:                                                          # as training.py: the raw entry point with h8[7] set
            oc.t += 1
            c4, h8 = step_scalars(oc.opt, oc.table, oc.t, hyp=oc.hyp)
            h8[7] = grad_scale
            rt.check(oc.lib.aware_opt_clamp_step(oc.opt["kind"], rt._ptr(mine), rt._ptr(g), rt._ptr(oc.s1), rt._ptr(oc.s2),
                                                 rt._ptr(dlo), rt._ptr(dhi), n, c4.ctypes.data_as(C.POINTER(C.c_float)),
                                                 h8.ctypes.data_as(C.POINTER(C.c_float)), rt._stream()), "aware_opt_clamp_step")
        got = mine.cpu().double().numpy()
        err = np.abs(got - want[i]) / np.abs(want[i])
        worst = max(worst, float(err.max()))
        inside = (want[i] > lo64) & (want[i] < hi64)
        if inside.any():
            inner = max(inner, float(err[inside].max()))
    moved = float(np.abs(want[-1] - p0.double().numpy()).max())
    on_box = float(((want[-1] == lo64) | (want[-1] == hi64)).mean())
    print(f"{name} + {sched} n={n}: max relative difference over {steps} steps {worst:.2e} (inside the box {inner:.2e}); "
          f"moved by up to {moved:.2e}; {100 * on_box:.1f} % on the box at the end")
    assert moved > 1e-3
    assert on_box <= ON_BOX_CAP, on_box
    if on_box_over is not None:
        assert on_box > on_box_over, on_box
    assert worst < 3e-6, worst
    assert inner < 3e-6, inner
    return worst


@pytest.mark.parametrize("name,params,sched,sparams", CASES)
def test_registry_optimizers_match_torch_optim(rt, name, params, sched, sparams):
    """25 steps of every optimiser the reference's registry can run, with and without a learning-rate scheduler, as ONE
    device kernel per step (aware_opt_clamp_step: update + clamp) against torch.optim + torch.clamp on the CPU with the same
    gradients (embedding/multibit_embedder.py:85-86,112-117).  Tolerance: a few f32 roundings per step (the CPU kernels
    fuse / order a handful of operations differently)."""
    _seam(rt, name, params, sched, sparams, 5000, 25)


def _seam_id(c):
    return f"{case_id(c[:3])}-{c[3]}"


@pytest.mark.parametrize("case", seam_cases(), ids=_seam_id)
def test_registry_matrix_matches_torch_optim(rt, case):
    """The same over the matrix of tests/test_registry_host.py: every optimiser with every table scheduler it accepts
    (CyclicLR cycling the momentum of SGD and RMSprop and beta1 of the Adam family, and with cycle_momentum=False), the
    weight-decay / momentum / beta option sets without a scheduler -- L2 decay of RMSprop, Adagrad, Adamax and Adadelta and
    RMSprop with momentum among them -- at n = 1, 255, 257 and 5000."""
    name, k, skey, n = case
    params = OPTIONS[name][k]
    sched, sparams = scheduler_params(skey, params["lr"])
    _seam(rt, name, params, sched, sparams, n, 25, on_box_over=0.02 if _seam_id(case) in CLAMP_EXERCISED else None)


@pytest.mark.parametrize("bounds", ["lo", "hi", "none"])
def test_registry_one_sided_and_absent_bounds(rt, bounds):
    """lo = None, hi = None or both (the null-pointer branches of opt_clamp_kernel): torch.clamp on one side, or no clamp.
    Without a lower bound nothing keeps a parameter away from zero, where the relative error has no meaning: the rates keep
    the total move below the smallest parameter (0.1)."""
    name = {"lo": "adam", "hi": "rmsprop", "none": "sgd"}[bounds]
    params = {"adam": {"lr": 0.05}, "rmsprop": {"lr": 0.001}, "sgd": {"lr": 0.01, "momentum": 0.9}}[name]
    _seam(rt, name, params, "exponential", {"gamma": 0.97}, 5000, 25, bounds=bounds)


@pytest.mark.parametrize("name,params", [("adam", {"lr": 0.02}), ("sgd", {"lr": 0.05, "momentum": 0.9, "weight_decay": 0.01})])
def test_registry_gradient_scale_slot(rt, name, params):
    """h8[7] = 1/7 (the gradient-scale slot the trainer uses for a summed batch gradient) against torch fed grad / 7: Adam
    as the trainer runs it, and SGD with L2 decay, where the scale has to come before the decay."""
    _seam(rt, name, params, "step", {"step_size": 5, "gamma": 0.7}, 5000, 25, grad_scale=1.0 / 7.0)


def test_registry_grid_stride_loop(rt):
    """n = 4096 * 256 + 257: the launch is capped at 4096 workgroups, so every thread of the first 257 takes the grid-stride
    loop twice.  RMSprop with momentum (both state arrays), 3 steps."""
    _seam(rt, "rmsprop", {"lr": 0.002, "momentum": 0.9}, None, None, 4096 * 256 + 257, 3)


@pytest.fixture(scope="module")
def O():
    from oracle import aware_oracle
    return aware_oracle


# ---- the session's optimiser step (opt_rows_kernel), one step at a time -----------------------------------------------------

LENGTHS = [16000, 5000, 20000]          # 63, 20 and 79 frames: the kernel's binary search over frame_off has three clips to find
CARD_BAND = (32, 256)                   # the model card's band: 225 columns in rows of 256 (the early-return lanes)
WIDE_BAND = (0, 512)                    # 513 columns in rows of 576: three passes of the column loop, the last one partial
NO_SCHED = ("reduce_lr_on_plateau", {"factor": 0.9, "patience": 500})       # cannot fire: a constant rate
FIRING = ("reduce_lr_on_plateau", {"factor": 0.5, "patience": 0, "threshold": 0.1, "min_lr": 0.008})
STEP_BOUND = 3e-6                       # the seam kernel's bound: the same arithmetic, one step instead of 25 carried
STEP_BOUND_CAP = 2e-4                   # the fused test's bound: no allowance for an unrepeatable gradient may pass it

# in-band |c| of these clips: median ~3.9 (1 % quantile 0.45); first gradients: median ~4e-5.  Learning rates are chosen so
# that the median element moves by >= 1e-3 relative per step while <= 30 % of the elements end on the box; L2 weight decay
# of 1e-5 makes wd * c comparable to the gradient.  Every scheduler event falls inside 12 steps.  The L2 cases of the
# adaptive kinds take eps = 1e-6: g + wd * c cancels to within a float32 rounding of g (2e-12) for a few elements per step,
# and the first steps' update lr * g / (|g| + eps) turns that into lr * 2e-12 / eps -- 2e-5 at torch's default eps of 1e-8, a
# property of float32 and not of the kernel; at 1e-6 it is 2e-7.
SESSION_CASES = {
    "adam-cosine": ("adam", {"lr": 0.05}, "cosine_annealing", {"T_max": 5, "eta_min": 0.01}),
    "adamw-exponential": ("adamw", {"lr": 0.05, "weight_decay": 0.01}, "exponential", {"gamma": 0.9}),
    "sgd-step": ("sgd", {"lr": 300.0, "momentum": 0.9}, "step", {"step_size": 4, "gamma": 0.5}),
    "sgd_nesterov-multi_step": ("sgd", {"lr": 300.0, "momentum": 0.8, "nesterov": True, "weight_decay": 1e-5},
                                "multi_step", {"milestones": [3, 7], "gamma": 0.6}),
    "sgd_dampening-warm_restarts": ("sgd", {"lr": 400.0, "momentum": 0.7, "dampening": 0.2},
                                    "cosine_annealing_warm_restarts", {"T_0": 3, "T_mult": 2, "eta_min": 100.0}),
    "rmsprop-plateau": ("rmsprop", {"lr": 0.03},) + FIRING,
    "rmsprop_l2-step": ("rmsprop", {"lr": 0.02, "weight_decay": 1e-5, "alpha": 0.9, "eps": 1e-6}, "step", {"step_size": 4, "gamma": 0.5}),
    "rmsprop-cyclic": ("rmsprop", {"lr": 0.004}, "cyclic", {"base_lr": 0.002, "max_lr": 0.006, "step_size_up": 2, "step_size_down": 3}),
    "rmsprop_momentum-none": ("rmsprop", {"lr": 0.004, "momentum": 0.6},) + NO_SCHED,
    "adagrad-multi_step": ("adagrad", {"lr": 0.1, "lr_decay": 0.05}, "multi_step", {"milestones": [3, 7], "gamma": 0.6}),
    "adagrad_l2-none": ("adagrad", {"lr": 0.1, "weight_decay": 1e-5, "eps": 1e-6},) + NO_SCHED,
    "adamax-cyclic": ("adamax", {"lr": 0.05}, "cyclic", {"base_lr": 0.02, "max_lr": 0.06, "step_size_up": 2, "step_size_down": 3}),
    "adamax_l2-exponential": ("adamax", {"lr": 0.05, "weight_decay": 1e-5, "eps": 1e-6}, "exponential", {"gamma": 0.9}),
    "adadelta-cosine": ("adadelta", {"lr": 1000.0}, "cosine_annealing", {"T_max": 5, "eta_min": 300.0}),
    "adadelta_l2-warm_restarts": ("adadelta", {"lr": 1000.0, "weight_decay": 1e-5, "rho": 0.8},
                                  "cosine_annealing_warm_restarts", {"T_0": 3, "T_mult": 2, "eta_min": 300.0}),
    "nadam-exponential_1": ("nadam", {"lr": 0.1}, "exponential", {"gamma": 1.0}),       # the card's optimiser through opt_rows_kernel
    "nadam_l2-plateau": ("nadam", {"lr": 0.1, "weight_decay": 1e-5, "eps": 1e-6}, "reduce_lr_on_plateau",
                         {"factor": 0.5, "patience": 1, "threshold": 0.1, "min_lr": 0.02}),
}
SESSION_RUNS = [(k, CARD_BAND) for k in SESSION_CASES] + [("adam-cosine", WIDE_BAND), ("rmsprop-plateau", WIDE_BAND)]

_PLANS, _DETS, _AUDIO = {}, {}, {}


def _plan_det(rt, O, band):
    if band not in _PLANS:
        _PLANS[band] = rt.Plan() if band == CARD_BAND else rt.Plan(band_bins=band)
        ws, bs = O.detector_weights()
        _DETS[band] = rt.DetectorWeights(_PLANS[band], O.mel_filter_bank(), [w.numpy() for w in ws], [b.numpy() for b in bs])
    return _PLANS[band], _DETS[band]


def _clips(rt, seed=800):
    if seed not in _AUDIO:
        clips = [make_clip(seed + i, l) for i, l in enumerate(LENGTHS)]
        batch = rt.Batch(LENGTHS)
        wm = np.stack([(2 * b - 1).astype(np.float32) for _, b in clips])
        _AUDIO[seed] = (batch, batch.pack([c for c, _ in clips]), torch.from_numpy(wm).cuda())
    return _AUDIO[seed]


def _registry_session(rt, O, band, num_iterations, name, params, sched, sparams, use_graph=False, seed=800):
    """An embed session with an optimiser / scheduler of the registries, begun on the ragged batch."""
    from aware_amd.embedding.optimizers import get_optimizer
    from aware_amd.embedding.schedulers import get_scheduler
    plan, det = _plan_det(rt, O, band)
    batch, audio, wm = _clips(rt, seed)
    sess = rt.EmbedSession(plan, det, batch, num_iterations=num_iterations, use_graph=use_graph)
    opt = get_optimizer(name, None, **params)
    sess.set_optimizer(opt, get_scheduler(sched, opt, num_iterations, **sparams))
    sess.begin(audio, wm)
    return sess, batch


def host_schedulers(name, params, sched, sparams, tensors):
    """One float64 torch optimiser + scheduler per clip, as the reference runs them (one clip at a time)."""
    opts = [TORCH_OPT[name]([t], **params) for t in tensors]
    if sched == "reduce_lr_on_plateau":
        scheds = [SCH.ReduceLROnPlateau(o, **sparams) for o in opts]
    else:
        scheds = [TORCH_SCHED[sched](o, **sparams) for o in opts]
    return opts, scheds


def check_session_steps(sess, frame_offsets, nb, name, params, sched, sparams, steps, table=None, tolerance_db=6.0):
    """`steps` iterations of a session whose optimiser steps in opt_rows_kernel, each against ONE step of float64 torch.optim
    (its state carried on the host, the parameters restarted from the device's coefficients) on the gradient the session
    reports at the same point, at the rate of torch's own scheduler (one per clip, ReduceLROnPlateau fed the device's
    losses), clamped to the box recomputed from c0.  Also: the table's / the device's per-clip rate equals torch's, the
    best snapshot (pre-step loss, post-clamp coefficients, per clip) bit for bit, zero columns beyond the band, the step
    counter.  Returns (worst error, worst error inside the box, share on the box at the end, gradient spread)."""
    B = len(frame_offsets) - 1
    fo = frame_offsets
    c0 = sess.coef.cpu().double().clone()
    d = c0 * 10 ** (-tolerance_db / 20)
    lo, hi = (c0 - d).clamp_min(0), c0 + d
    P = [c0[fo[i]:fo[i + 1], :nb].clone().requires_grad_(True) for i in range(B)]
    opts, scheds = host_schedulers(name, params, sched, sparams, P)
    best_loss = np.full(B, np.inf)
    best = c0.clone()
    worst = inner = spread = 0.0
    rates_differed = False
    for it in range(steps):
        pre = sess.coef.cpu().double().clone()
        g = sess.gradient().cpu()
        g2 = sess.gradient().cpu()
        loss = sess.loss.cpu().numpy().copy()
        lrs = sess.clip_learning_rates().copy()
        rates_differed |= len(set(lrs.tolist())) > 1
        step0 = int(sess.step.cpu()[0])
        sess.iterate(1)
        got = sess.coef.cpu().double().clone()
        assert int(sess.step.cpu()[0]) == step0 + 1
        want = pre.clone()
        allowance = 0.0
        for i in range(B):
            rows = slice(fo[i], fo[i + 1])
            lr = opts[i].param_groups[0]["lr"]
            if sched == "reduce_lr_on_plateau":
                np.testing.assert_allclose(lrs[i], lr, rtol=1e-12)               # the device's per-clip rate
            elif table is not None:
                np.testing.assert_allclose(table[it, 3], lr, rtol=1e-12)         # the rate the host baked into the table
            results = []
            for grad in ([g, g2] if not torch.equal(g, g2) else [g]):
                o = opts[i] if grad is g else copy.deepcopy(opts[i])             # (the second gradient steps a copy)
                p = o.param_groups[0]["params"][0]
                with torch.no_grad():
                    p.copy_(pre[rows, :nb])
                p.grad = grad[rows, :nb].double()
                o.step()
                results.append(torch.minimum(torch.maximum(p.detach(), lo[rows, :nb]), hi[rows, :nb]).clone())
            want[rows, :nb] = results[0]
            if len(results) > 1:
                allowance = max(allowance, float(((results[0] - results[1]).abs() / (1e-3 + results[0].abs())).max()))
            scheds[i].step(float(loss[i])) if sched == "reduce_lr_on_plateau" else scheds[i].step()
        spread = max(spread, allowance)
        bound = STEP_BOUND + allowance
        assert bound <= STEP_BOUND_CAP, (it, allowance)
        err = ((got - want).abs() / (1e-3 + want.abs()))[:, :nb]
        inside = ((want > lo) & (want < hi))[:, :nb]
        moved = float(((want - pre).abs() / pre.abs())[:, :nb].median())
        worst, inner = max(worst, float(err.max())), max(inner, float(err[inside].max()))
        assert moved >= 1e-3, (it, moved)
        assert float(err.max()) < bound, (it, float(err.max()), bound)
        assert float(err[inside].max()) < bound, (it, float(err[inside].max()), bound)
        assert float(got[:, nb:].abs().max()) == 0.0
        for i in range(B):
            if loss[i] < best_loss[i]:
                best_loss[i] = loss[i]
                best[fo[i]:fo[i + 1]] = got[fo[i]:fo[i + 1]]
        np.testing.assert_array_equal(sess.best_coef.cpu().double().numpy(), best.numpy())
    on_box = float((~inside).double().mean())
    assert on_box <= ON_BOX_CAP, on_box
    if sched == "reduce_lr_on_plateau" and sparams["patience"] < steps:
        assert rates_differed                                            # ... so a wrong clip lookup of the rate would show
    return worst, inner, on_box, spread


@pytest.mark.parametrize("key,band", SESSION_RUNS, ids=[f"{k}-{b[0]}_{b[1]}" for k, b in SESSION_RUNS])
def test_session_optimizer_steps_match_torch_optim(rt, O, key, band):
    """12 iterations of a registry session on a ragged batch (63, 20 and 79 frames), every step of opt_rows_kernel against one
    float64 torch.optim step (check_session_steps): all 8 kinds, every scheduler, the L2 weight-decay variants, AdamW's
    decoupled decay, Nesterov and dampened SGD, RMSprop with cycled and with fixed momentum, per-clip rates of a firing
    ReduceLROnPlateau; on the model card's band (225 columns of 256) and, for two kinds, on (0, 512) (513 columns of 576).
    Bound 3e-6 on |got - want| / (1e-3 + |want|) (plus what an unrepeatable gradient() would account for, never above 2e-4).
    NAdam + exponential(gamma=1): the card's optimiser forced through opt_rows_kernel, whose first step also agrees with a
    fused-NAdam session on the same clips under that test's 2e-4."""
    name, params, sched, sparams = SESSION_CASES[key]
    steps = 12
    sess, batch = _registry_session(rt, O, band, steps, name, params, sched, sparams)
    nb = band[1] - band[0] + 1
    assert sess.plan.band_stride == (256 if band == CARD_BAND else 576)
    g, g2 = sess.gradient(), sess.gradient()
    assert torch.equal(g, g2)                                            # the gradient inside iterate() is the one reported
    if key == "nadam-exponential_1":
        plan, det = _plan_det(rt, O, band)
        _, audio, wm = _clips(rt)
        fused = rt.EmbedSession(plan, det, batch, num_iterations=steps, use_graph=False, lr=params["lr"])
        fused.begin(audio, wm)
        fused.iterate(1)
        fused_coef = fused.coef.cpu().double().clone()
    worst, inner, on_box, spread = check_session_steps(sess, batch.frame_offsets, nb, name, params, sched, sparams, steps,
                                                       table=sess._opt_table)
    print(f"{key} band {band}: max step error {worst:.2e} (inside the box {inner:.2e}); {100 * on_box:.1f} % on the box after "
          f"{steps} steps; gradient spread {spread:.1e}")
    if sched == "reduce_lr_on_plateau" and sparams["patience"] < steps:
        lrs = sess.clip_learning_rates()
        assert lrs.min() < params["lr"]                                  # ... the scheduler fired
    if key == "nadam-exponential_1":
        again, _ = _registry_session(rt, O, band, steps, name, params, sched, sparams)
        again.iterate(1)
        first = again.coef.cpu().double()
        err = float(((first - fused_coef).abs() / (1e-3 + fused_coef.abs()))[:, :nb].max())
        print(f"first step of opt_rows_kernel NAdam against the fused epilogue: {err:.2e}")
        assert err < 2e-4, err
    with pytest.raises(ValueError):
        sess.iterate(1)                                                  # the table holds num_iterations steps


# ---- graph replay and reset of a registry session ---------------------------------------------------------------------------

def _state(sess):
    torch.cuda.synchronize()
    return {"coef": sess.coef.cpu().clone(), "best_coef": sess.best_coef.cpu().clone(), "loss": sess.loss.cpu().clone(),
            "best_loss": sess.best_loss.cpu().clone(), "lr": torch.from_numpy(sess.clip_learning_rates().copy())}


@pytest.mark.parametrize("key", ["adam-cosine", "rmsprop-plateau"])
def test_registry_session_graph_replay_and_reset(rt, O, key):
    """iterate(20) of a registry session as graph replays (one 16-body graph, four single bodies) against 20 plain launches:
    coefficients, best snapshot, losses, best losses and per-clip rates bit for bit; a 21st step is refused; a second begin()
    on the same session repeats the first run bit for bit (moments, step counter, plateau state and per-clip rates reset)."""
    name, params, sched, sparams = SESSION_CASES[key]
    n = 20
    if sched == "cosine_annealing":
        sparams = dict(sparams, T_max=8)
    graph, _ = _registry_session(rt, O, CARD_BAND, n, name, params, sched, sparams, use_graph=True)
    graph.iterate(n)
    a = _state(graph)
    plain, _ = _registry_session(rt, O, CARD_BAND, n, name, params, sched, sparams, use_graph=False)
    plain.iterate(n)
    b = _state(plain)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert int(graph.step.cpu()[0]) == int(plain.step.cpu()[0])
    if sched == "reduce_lr_on_plateau":
        assert float(a["lr"].min()) < params["lr"]                       # the plateau state did something
    for sess in (graph, plain):
        with pytest.raises(ValueError):
            sess.iterate(1)
    _, audio, wm = _clips(rt)
    graph.begin(audio, wm)
    graph.iterate(n)
    c = _state(graph)
    for k in a:
        assert torch.equal(a[k], c[k]), k


# ---- ReduceLROnPlateau on the device ------------------------------------------------------------------------------------------

# (patience 0 with a threshold of 0.1 halves every clip's rate at every step -- these losses improve by about 3 % per step --
# so no two clips would ever differ; at 0.03 some steps count as improvements and the clips part ways from the third step on)
PLATEAU_SETS = {
    "patience0": {"factor": 0.5, "patience": 0, "threshold": 0.03},
    "patience1_min_lr": {"factor": 0.5, "patience": 1, "threshold": 0.1, "min_lr": 0.05 / 3},
    "below_eps": {"factor": 0.999999, "patience": 0, "eps": 1e-3},
}


@pytest.mark.parametrize("key", list(PLATEAU_SETS))
def test_plateau_kernel_follows_torch_on_device_losses(rt, O, key):
    """16 iterations of a ragged three-clip session with ReduceLROnPlateau: the DEVICE's per-clip losses fed to one torch
    ReduceLROnPlateau per clip on the CPU (no dependence on trajectory drift), the device's per-clip rates equal to torch's
    before every step and after the last.  Non-vacuity from torch's side: a reduction, clips at different rates, min_lr
    reached, or -- reductions below eps -- no change at all."""
    lr0, n = 0.05, 16
    kw = PLATEAU_SETS[key]
    sess, batch = _registry_session(rt, O, CARD_BAND, n, "adam", {"lr": lr0}, "reduce_lr_on_plateau", kw)
    B = batch.B
    stand_ins = [torch.nn.Parameter(torch.zeros(1)) for _ in range(B)]
    opts, scheds = host_schedulers("adam", {"lr": lr0}, "reduce_lr_on_plateau", kw, stand_ins)
    seen = []
    for it in range(n):
        want = np.asarray([o.param_groups[0]["lr"] for o in opts])
        np.testing.assert_allclose(sess.clip_learning_rates(), want, rtol=1e-12)
        seen.append(want)
        sess.iterate(1)
        loss = sess.loss.cpu().numpy()
        for i in range(B):
            opts[i].step()
            scheds[i].step(float(loss[i]))
    want = np.asarray([o.param_groups[0]["lr"] for o in opts])
    np.testing.assert_allclose(sess.clip_learning_rates(), want, rtol=1e-12)
    seen = np.stack(seen + [want])
    print(f"{key}: per-clip rates {seen[0]} -> {seen[-1]}")
    if key == "below_eps":
        assert (seen == lr0).all()
    else:
        assert seen.min() < lr0
        assert any(len(set(row)) > 1 for row in seen)
    if key == "patience1_min_lr":
        assert (seen == kw["min_lr"]).any() and seen.min() == kw["min_lr"]


EMBED_CASES = [
    ("adam", {"lr": 0.05}, "cosine_annealing", {"T_max": 30}),
    ("sgd", {"lr": 20.0, "momentum": 0.9}, "step", {"step_size": 10, "gamma": 0.5}),
    ("adamw", {"lr": 0.05, "weight_decay": 0.001}, "exponential", {"gamma": 0.97}),
    ("nadam", {"lr": 0.1}, "reduce_lr_on_plateau", {"factor": 0.5, "patience": 1, "threshold": 0.1}),
    ("rmsprop", {"lr": 0.02}, "reduce_lr_on_plateau", {"factor": 0.9, "patience": 500}),
]


@pytest.mark.parametrize("name,params,sched,sparams", EMBED_CASES)
def test_embed_session_with_registry_optimizer(rt, O, name, params, sched, sparams):
    """Embed sessions configured through the registries (AWAREEmbedder(optimizer_cfg=..., scheduler_cfg=...), the YAML strings of
    cards/config.yaml:17-26) against the oracle's registry loop (torch.optim on the CPU as the reference runs it, one clip at a
    time): 30 iterations of two clips, per-step losses within the 20-step drift band, the per-clip learning rates of a FIRING
    ReduceLROnPlateau equal to torch's."""
    from aware_amd.embedding import AWAREEmbedder
    steps = 30
    emb = AWAREEmbedder(num_iterations=steps, optimizer_cfg={"name": name, "params": params},
                        scheduler_cfg={"name": sched, "params": sparams}, loss="push_extremes", verbose=False, use_graph=True)
    lengths = [16000, 20000]
    pairs = [make_clip(400 + i, n) for i, n in enumerate(lengths)]
    wm = np.stack([O.bits_to_bipolar(p[1]) for p in pairs]).astype(np.float32)
    batch = rt.Batch(lengths)
    sess = emb.start_session(batch, 16000)
    sess.begin(batch.pack([p[0] for p in pairs]), torch.from_numpy(wm).cuda())
    mine, lrs = [], []
    for _ in range(steps):
        if sched == "reduce_lr_on_plateau" and sparams["patience"] < steps:
            lrs.append(sess.clip_learning_rates().copy())
        sess.iterate(1)
        mine.append(sess.loss.cpu().numpy().copy())
    mine = np.stack(mine)
    for i, (clip, _) in enumerate(pairs):
        ref = O.Embedder(num_iterations=steps, optimizer=name, optimizer_params=params, scheduler=sched, scheduler_params=sparams)
        rl, rlr = [], []
        ref.embed_registry(clip[None], wm[i][None], record=lambda it, l, lr: (rl.append(l), rlr.append(lr)))
        d = np.abs(mine[:, i] - np.asarray(rl))
        print(f"{name} + {sched}, clip {i}: |loss - oracle| step0 {d[0]:.1e} max {d.max():.2e}; loss {rl[0]:.4f} -> {rl[-1]:.4f}; "
              f"lr {rlr[0]:.4g} -> {rlr[-1]:.4g}")
        assert d[0] < 2e-5 and d.max() < 3 * 1.9e-3, d
        assert rl[-1] < rl[0] - 0.01                                   # the optimiser works on the loss
        if lrs:
            np.testing.assert_allclose(np.asarray(lrs)[:, i], np.asarray(rlr), rtol=1e-12)
            assert rlr[-1] < rlr[0]                                    # ... and the scheduler fired
