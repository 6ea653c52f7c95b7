"""The host half of the optimiser / scheduler registries (aware_amd/embedding/{optimizers,schedulers}.py) without a GPU:
a float32 numpy restatement of csrc/dsp_args.hpp::opt_clamp_update (all 8 kinds, the kernel's operation order) driven by
step_table / step_scalars, against float64 torch.optim + torch.clamp over the whole optimiser x option x scheduler matrix;
the refusals; and a float64 restatement of csrc/seam_kernels.hip::plateau_kernel against torch's ReduceLROnPlateau.

The matrix, the input recipe and the float64 reference are shared with tests/test_gpu_registry.py, which runs the device
kernels over the same cases."""
import itertools
import math

import numpy as np
import pytest
import torch

F = np.float32
SCH = torch.optim.lr_scheduler
TORCH_OPT = {"adam": torch.optim.Adam, "nadam": torch.optim.NAdam, "sgd": torch.optim.SGD, "rmsprop": torch.optim.RMSprop,
             "adagrad": torch.optim.Adagrad, "adadelta": torch.optim.Adadelta, "adamax": torch.optim.Adamax, "adamw": torch.optim.AdamW}
TORCH_SCHED = {"cosine_annealing": SCH.CosineAnnealingLR, "cosine_annealing_warm_restarts": SCH.CosineAnnealingWarmRestarts,
               "step": SCH.StepLR, "multi_step": SCH.MultiStepLR, "exponential": SCH.ExponentialLR, "cyclic": SCH.CyclicLR}

# option sets per optimiser: [0] is the plain one, the others the weight-decay / momentum / beta variants
OPTIONS = {
    "nadam": [{"lr": 0.1}, {"lr": 0.03, "weight_decay": 0.01, "momentum_decay": 0.01}],
    "adam": [{"lr": 0.02}, {"lr": 0.01, "betas": (0.8, 0.99), "weight_decay": 0.01, "eps": 1e-6}],
    "adamw": [{"lr": 0.03, "weight_decay": 0.1}, {"lr": 0.02, "betas": (0.85, 0.98), "weight_decay": 0.0}],
    "sgd": [{"lr": 0.05}, {"lr": 0.05, "momentum": 0.9, "nesterov": True, "weight_decay": 0.01},
            {"lr": 0.05, "momentum": 0.7, "dampening": 0.2}, {"lr": 0.05, "weight_decay": 0.02}],
    "rmsprop": [{"lr": 0.01, "alpha": 0.95}, {"lr": 0.005, "weight_decay": 0.01}, {"lr": 0.002, "momentum": 0.9},
                {"lr": 0.002, "momentum": 0.5, "weight_decay": 0.01, "eps": 1e-6}],
    "adagrad": [{"lr": 0.1, "lr_decay": 0.05}, {"lr": 0.05, "weight_decay": 0.01}],
    "adamax": [{"lr": 0.02}, {"lr": 0.01, "betas": (0.8, 0.99), "weight_decay": 0.01}],
    "adadelta": [{"lr": 1.0, "rho": 0.85}, {"lr": 1.0, "weight_decay": 0.01}],
}
SCHEDULERS = [None, "cosine_annealing", "cosine_annealing_warm_restarts", "step", "multi_step", "exponential", "cyclic",
              "cyclic_fixed_momentum"]
NO_CYCLED_MOMENTUM = ("adagrad", "adadelta")      # neither momentum nor beta1: torch's CyclicLR(cycle_momentum=True) refuses


def scheduler_params(sched, lr):
    """(registry name, keyword arguments) of a scheduler of the matrix; every event falls inside 25 steps."""
    if sched is None:
        return None, None
    cyc = {"base_lr": lr / 4, "max_lr": lr * 1.5, "step_size_up": 3, "step_size_down": 5}
    return {"cosine_annealing": ("cosine_annealing", {"T_max": 12, "eta_min": lr * 1e-2}),
            "cosine_annealing_warm_restarts": ("cosine_annealing_warm_restarts", {"T_0": 6, "T_mult": 2}),
            "step": ("step", {"step_size": 5, "gamma": 0.7}),
            "multi_step": ("multi_step", {"milestones": [4, 11], "gamma": 0.5}),
            "exponential": ("exponential", {"gamma": 0.95}),
            "cyclic": ("cyclic", cyc),
            "cyclic_fixed_momentum": ("cyclic", dict(cyc, cycle_momentum=False))}[sched]


def matrix():
    """(optimiser, option index, scheduler key) of every combination torch accepts."""
    out = []
    for name, sets in OPTIONS.items():
        for k, sched in itertools.product(range(len(sets)), SCHEDULERS):
            if sched == "cyclic" and name in NO_CYCLED_MOMENTUM:
                continue
            out.append((name, k, sched))
    return out


def seam_cases():
    """The cases the device kernel runs (tests/test_gpu_registry.py): the first option set of every optimiser with every
    scheduler it accepts, the other option sets without one; n rotates over {5000, 1, 255, 257} (one element, one short of a
    workgroup, one past it, 20 workgroups) -- the weight-decay sets skip n = 1, where one element decides the whole share of
    elements on the box.  [(optimiser, option index, scheduler key, n)]"""
    out = []
    for name, sets in OPTIONS.items():
        for sched in SCHEDULERS:
            if not (sched == "cyclic" and name in NO_CYCLED_MOMENTUM):
                out.append((name, 0, sched, (5000, 1, 255, 257)[len(out) % 4]))
        for k in range(1, len(sets)):
            out.append((name, k, None, (5000, 255, 257)[len(out) % 3]))
    return out


def case_id(c):
    return f"{c[0]}{c[1]}-{c[2] or 'none'}"


def make_inputs(name, n, steps):
    """Parameters in [0.1, 2.1), the box [0.5, 1.5] * p0 and `steps` gradients of growing size (the recipe of the seam test)."""
    g = torch.Generator().manual_seed(len(name) + steps)
    p0 = torch.rand(n, generator=g) * 2 + 0.1
    grads = [torch.randn(n, generator=g) * (0.5 + 0.1 * i) * 1e-2 for i in range(steps)]
    return p0, p0 * 0.5, p0 * 1.5, grads


def torch_reference(name, params, sched, sparams, p0, grads, lo=None, hi=None, grad_scale=1.0):
    """float64 torch.optim + scheduler + torch.clamp, the reference's loop (embedding/multibit_embedder.py:85-86,112-117):
    the parameters after every step, [steps][n] float64."""
    ref = p0.double().clone().requires_grad_(True)
    topt = TORCH_OPT[name]([ref], **params)
    tsch = TORCH_SCHED[sched](topt, **sparams) if sched else None
    lo = None if lo is None else lo.double()
    hi = None if hi is None else hi.double()
    out = []
    for g in grads:
        ref.grad = g.double() * grad_scale
        topt.step()
        if tsch is not None:
            tsch.step()
        if lo is not None or hi is not None:
            with torch.no_grad():
                ref.data = torch.clamp(ref.data, lo, hi)
        out.append(ref.detach().clone().numpy())
    return np.stack(out)


def opt_clamp_update_np(kind, p, mo, ve, g, lo, hi, c, h):
    """csrc/dsp_args.hpp::opt_clamp_update in float32 numpy, operation for operation.  p, mo, ve, g: float32 arrays; lo, hi:
    float32 arrays or None; c: 4 and h: 8 float32 scalars.  Returns the new (p, mo, ve)."""
    c = [F(x) for x in c]
    h = [F(x) for x in h]
    assert p.dtype == mo.dtype == ve.dtype == g.dtype == F
    if h[7] != 0:
        g = g * h[7]
    if kind == 2:
        p = p * c[3]
    elif h[4] != 0:
        g = g + h[4] * p
    if kind == 0:
        mo = mo + h[0] * (g - mo)
        ve = ve * h[1] + (h[2] * g) * g
        den = np.sqrt(ve / c[2]) + h[3]
        p = p + (c[0] * g) / den
        p = p + (c[1] * mo) / den
    elif kind in (1, 2):
        mo = mo + h[0] * (g - mo)
        ve = ve * h[1] + (h[2] * g) * g
        den = np.sqrt(ve) / c[2] + h[3]
        p = p + (c[0] * mo) / den
    elif kind == 3:
        d = g
        if h[0] != 0:
            mo = g.copy() if c[1] != 0 else mo * h[0] + h[6] * g
            d = g + h[0] * mo if h[5] != 0 else mo
        p = p + c[0] * d
    elif kind == 4:
        ve = ve * h[1] + (h[2] * g) * g
        avg = np.sqrt(ve) + h[3]
        if h[0] != 0:
            mo = mo * h[0] + g / avg
            p = p + c[0] * mo
        else:
            p = p + (c[0] * g) / avg
    elif kind == 5:
        ve = ve + g * g
        sd = np.sqrt(ve) + h[3]
        p = p + (c[0] * g) / sd
    elif kind == 6:
        mo = mo + h[0] * (g - mo)
        ve = np.maximum(ve * h[1], np.abs(g) + h[3])
        p = p + (c[0] * mo) / ve
    else:
        assert kind == 7
        ve = ve * h[1] + (h[2] * g) * g
        sd = np.sqrt(ve + h[3])
        delta = np.sqrt(mo + h[3]) / sd * g
        mo = mo * h[1] + (h[2] * delta) * delta
        p = p + c[0] * delta
    if lo is not None:
        p = np.maximum(p, lo)
    if hi is not None:
        p = np.minimum(p, hi)
    assert p.dtype == mo.dtype == ve.dtype == F
    return p, mo, ve


def restated_trajectory(name, params, sched, sparams, p0, grads, lo, hi):
    """What runtime.OptClamp does, with the kernel replaced by its restatement: hyper-parameters before the table, the table
    over a fresh scheduler, step_scalars per step."""
    from aware_amd.embedding.optimizers import get_optimizer, hyper_parameters, step_scalars, step_table
    from aware_amd.embedding.schedulers import get_scheduler
    steps = len(grads)
    opt = get_optimizer(name, None, **params)
    sd = get_scheduler(sched, opt, steps, **sparams) if sched else None
    hyp = hyper_parameters(opt)
    tab = step_table(opt, steps, sd["torch"] if sd else None)
    p = p0.numpy().astype(F)
    mo, ve = np.zeros_like(p), np.zeros_like(p)
    lo, hi = lo.numpy().astype(F), hi.numpy().astype(F)
    out = []
    for t in range(1, steps + 1):
        c4, h8 = step_scalars(opt, tab, t, hyp=hyp)
        assert c4.dtype == h8.dtype == F
        p, mo, ve = opt_clamp_update_np(opt["kind"], p, mo, ve, grads[t - 1].numpy().astype(F), lo, hi, c4, h8)
        out.append(p)
    return np.stack(out), tab


@pytest.mark.parametrize("case", matrix(), ids=case_id)
def test_step_table_and_restated_kernel_match_torch(case):
    """25 carried steps of every optimiser x option set x table scheduler (none, the six of the registry, CyclicLR with
    cycle_momentum=False) the reference's registries can run: step_table + step_scalars + the float32 restatement of the
    kernel against float64 torch.optim + clamp with the same gradients, to the seam test's 3e-6 relative (a few float32
    roundings per step; the restatement alone measures <= 1.9e-6).  CyclicLR's default cycle_momentum=True cycles the
    momentum of SGD (from 0 as well) and RMSprop and beta1 of Adam / AdamW / NAdam / Adamax: the table carries it."""
    name, k, skey = case
    params = OPTIONS[name][k]
    sched, sparams = scheduler_params(skey, params["lr"])
    n, steps = 2000, 25
    p0, lo, hi, grads = make_inputs(name, n, steps)
    want = torch_reference(name, params, sched, sparams, p0, grads, lo, hi)
    got, tab = restated_trajectory(name, params, sched, sparams, p0, grads, lo, hi)
    err = float((np.abs(got - want) / np.abs(want)).max())
    moved = float(np.abs(want[-1] - p0.double().numpy()).max())
    print(f"{case_id(case)}: max relative difference over {steps} steps {err:.2e}; moved by up to {moved:.2e}")
    assert moved > 1e-3
    assert err < 3e-6, err
    if skey == "cyclic":
        assert tab[:, 4].min() >= 0 and tab[:, 4].max() > tab[:, 4].min()      # the cycled momentum / beta1 is in the table
    if name == "rmsprop" and params.get("momentum") and skey != "cyclic":
        assert tab[0, 4] == params["momentum"]


def test_cycled_momentum_reaches_the_table():
    """torch's CyclicLR(cycle_momentum=True) writes 0.8-0.9 into param_group['momentum'] of SGD(momentum=0) and RMSprop
    (momentum=0), and into beta1: the table's h0 follows torch's own group, step by step."""
    from aware_amd.embedding.optimizers import get_optimizer, step_table
    from aware_amd.embedding.schedulers import get_scheduler
    for name in ("sgd", "rmsprop", "adam", "adamw", "nadam", "adamax"):
        opt = get_optimizer(name, None, lr=0.01)
        sd = get_scheduler("cyclic", opt, 12, base_lr=0.001, max_lr=0.01, step_size_up=2, step_size_down=3)
        tab = step_table(opt, 12, sd["torch"])
        stand_in = torch.nn.Parameter(torch.zeros(1))
        topt = TORCH_OPT[name]([stand_in], lr=0.01)
        tsch = SCH.CyclicLR(topt, base_lr=0.001, max_lr=0.01, step_size_up=2, step_size_down=3)
        for t in range(12):
            g = topt.param_groups[0]
            m = g["momentum"] if "momentum" in g else g["betas"][0]
            assert tab[t, 3] == g["lr"], (name, t)
            assert tab[t, 4] == (m if "momentum" in g else 1.0 - m), (name, t)
            topt.step()
            tsch.step()
        assert 0.8 <= (tab[:, 4].min() if name in ("sgd", "rmsprop") else 1 - tab[:, 4].max()) < 0.9 + 1e-12


def test_hyper_parameters_survive_the_table():
    """hyper_parameters taken before step_table is what the device gets: building the table (which steps a CyclicLR, which
    rewrites the group) leaves the snapshot alone, and step_scalars with the snapshot differs from the snapshot only in h[0]."""
    from aware_amd.embedding.optimizers import get_optimizer, hyper_parameters, step_scalars, step_table
    from aware_amd.embedding.schedulers import get_scheduler
    opt = get_optimizer("rmsprop", None, lr=0.01, alpha=0.9, weight_decay=0.1)
    hyp = hyper_parameters(opt)
    assert hyp[0][0] == 0.0
    sd = get_scheduler("cyclic", opt, 8, base_lr=0.001, max_lr=0.01, step_size_up=2)
    before = (list(hyp[0]), hyp[1])
    tab = step_table(opt, 8, sd["torch"])
    assert (list(hyp[0]), hyp[1]) == before
    for t in range(1, 9):
        c4, h8 = step_scalars(opt, tab, t, hyp=hyp)
        assert h8[0] == F(tab[t - 1, 4]) and 0.8 <= h8[0] <= 0.9
        np.testing.assert_array_equal(h8[1:], np.asarray(hyp[0][1:], dtype=F))
        assert c4[0] == F(-tab[t - 1, 3])
    assert (list(hyp[0]), hyp[1]) == before


def test_registry_refusals():
    """What cannot run on the device is refused with the error the module documents (or torch's own), never a silently wrong
    table."""
    from aware_amd.embedding.optimizers import get_optimizer
    from aware_amd.embedding.schedulers import get_scheduler
    for name in NO_CYCLED_MOMENTUM:
        with pytest.raises(ValueError):                          # torch: "optimizer must support momentum or beta1 ..."
            get_scheduler("cyclic", get_optimizer(name, None, lr=0.1), 25, base_lr=0.01, max_lr=0.1)
        assert get_scheduler("cyclic", get_optimizer(name, None, lr=0.1), 25, base_lr=0.01, max_lr=0.1,
                             cycle_momentum=False)["torch"] is not None
    for name, kw in (("adam", {"amsgrad": True}), ("adamw", {"amsgrad": True}), ("adam", {"maximize": True}),
                     ("sgd", {"maximize": True}), ("adadelta", {"maximize": True}), ("rmsprop", {"centered": True}),
                     ("rmsprop", {"centered": True, "momentum": 0.9}), ("adagrad", {"initial_accumulator_value": 0.1}),
                     ("sparse_adam", {}), ("lbfgs", {})):
        with pytest.raises(NotImplementedError):
            get_optimizer(name, None, **kw)
    with pytest.raises(ValueError, match="not found"):
        get_optimizer("nope", None, lr=0.1)
    with pytest.raises(ValueError, match="not found"):
        get_scheduler("nope", get_optimizer("adam", None, lr=0.1), 25)
    assert get_optimizer("rmsprop", None, lr=0.01, momentum=0.9)["group"]["momentum"] == 0.9     # on the device now


# ---- ReduceLROnPlateau ---------------------------------------------------------------------------------------------------

def plateau_np(loss, state, lr, p):
    """csrc/seam_kernels.hip::plateau_kernel for one clip, in python floats (float64).  loss: the float32 loss the device
    holds; state: [best, num_bad]; p: the "plateau" dict of get_scheduler.  Returns the new rate."""
    cur = float(F(loss))
    best, bad = state
    if cur < best * (1.0 - p["threshold"]):
        best, bad = cur, 0.0
    else:
        bad += 1.0
    if bad > float(p["patience"]):
        new = max(lr * p["factor"], p["min_lr"])
        if lr - new > p["eps"]:
            lr = new
        bad = 0.0
    state[0], state[1] = best, bad
    return lr


def _rng_losses(seed, n, start, slope, noise):
    rng = np.random.default_rng(seed)
    return [float(F(start + slope * i + noise * rng.standard_normal())) for i in range(n)]


PLATEAU_CASES = {
    # name: (lr, scheduler arguments, losses, expected events)
    "fires": (0.1, {"factor": 0.5, "patience": 1, "threshold": 0.1}, _rng_losses(0, 30, 1.0, -0.01, 0.02), "fires"),
    "min_lr_binds": (0.1, {"factor": 0.5, "patience": 0, "threshold": 0.1, "min_lr": 0.1 / 3},
                     [1.0] * 12, "min_lr"),
    "small_reduction_ignored": (0.1, {"factor": 0.999999, "patience": 0, "eps": 1e-3}, [1.0] * 12, "constant"),
    "reduction_just_above_eps": (0.1, {"factor": 0.5, "patience": 0, "eps": 0.02}, [1.0] * 12, "fires"),
    "threshold_zero": (0.1, {"factor": 0.5, "patience": 1, "threshold": 0.0},
                       [1.0, 0.9, 0.9, 0.9, 0.8999999, 0.9, 0.9, 0.7, 0.7, 0.7, 0.7], "fires"),
    "patience_zero": (0.1, {"factor": 0.7, "patience": 0, "threshold": 1e-4}, _rng_losses(1, 30, 1.0, -0.02, 0.05), "fires"),
    "negative_losses": (0.1, {"factor": 0.5, "patience": 1, "threshold": 0.1},
                        [-0.5, -0.6, -0.9, -0.85, -0.8, -0.95, -0.5, -0.4, -1.2, -1.1, -0.3, -0.2, -1.0], "fires"),
    "crossing_zero": (0.1, {"factor": 0.5, "patience": 0, "threshold": 0.1}, [0.3, 0.1, 0.0, 0.0, -0.05, -0.01, -0.2, -0.1, -0.1], "fires"),
    "nan_in_the_middle": (0.1, {"factor": 0.5, "patience": 1, "threshold": 0.1},
                          [1.0, 0.8, float("nan"), float("nan"), 0.7, 0.5, float("nan"), 0.5, 0.5, 0.5, 0.3], "fires"),
    "nan_first": (0.1, {"factor": 0.5, "patience": 0}, [float("nan"), 1.0, 0.5, 0.5, float("inf"), 0.4], "fires"),
}


@pytest.mark.parametrize("key", list(PLATEAU_CASES))
def test_plateau_restatement_matches_torch(key):
    """The restated plateau_kernel, fed the parameters get_scheduler hands to the device, against
    torch.optim.lr_scheduler.ReduceLROnPlateau stepped with the same losses after each optimiser step: the learning rate of
    every step EXACTLY equal (both are python-float arithmetic)."""
    from aware_amd.embedding.optimizers import get_optimizer
    from aware_amd.embedding.schedulers import get_scheduler
    lr0, kw, losses, expect = PLATEAU_CASES[key]
    sd = get_scheduler("reduce_lr_on_plateau", get_optimizer("adam", None, lr=lr0), 400, **kw)
    assert sd["torch"] is None and not sd["constant_lr"] and sd["plateau"] is not None
    stand_in = torch.nn.Parameter(torch.zeros(1))
    topt = torch.optim.Adam([stand_in], lr=lr0)
    tsch = SCH.ReduceLROnPlateau(topt, **kw)
    state, lr = [math.inf, 0.0], lr0
    seen = [lr0]
    for i, l in enumerate(losses):
        topt.step()
        tsch.step(l)
        lr = plateau_np(l, state, lr, sd["plateau"])
        assert lr == topt.param_groups[0]["lr"], (key, i, lr, topt.param_groups[0]["lr"])
        seen.append(lr)
    if expect == "fires":
        assert seen[-1] < lr0
    elif expect == "min_lr":
        assert seen[-1] == kw["min_lr"] and seen[-1] > lr0 * kw["factor"] ** 2
    else:
        assert all(s == lr0 for s in seen)


def test_plateau_that_cannot_fire_is_a_constant_rate():
    """never_fires (patience + 1 >= num_iterations; torch refuses factor == 1 before that test is reached) maps to constant_lr, and torch agrees: on the worst
    sequence (every loss non-finite, so every step counts as bad) no step of the run sees a reduced rate."""
    from aware_amd.embedding.optimizers import get_optimizer
    from aware_amd.embedding.schedulers import get_scheduler
    for n, kw in ((400, {"factor": 0.9, "patience": 500}), (10, {"factor": 0.5, "patience": 9}), (10, {"factor": 0.5, "patience": 12})):
        sd = get_scheduler("reduce_lr_on_plateau", get_optimizer("nadam", None, lr=0.1), n, **kw)
        assert sd["constant_lr"] and sd["plateau"] is None and sd["torch"] is None, kw
        stand_in = torch.nn.Parameter(torch.zeros(1))
        topt = torch.optim.NAdam([stand_in], lr=0.1)
        tsch = SCH.ReduceLROnPlateau(topt, **kw)
        for _ in range(n):
            assert topt.param_groups[0]["lr"] == 0.1              # the rate this step's optimiser.step() uses
            topt.step()
            tsch.step(float("nan"))
    with pytest.raises(ValueError):                               # torch itself refuses factor >= 1
        get_scheduler("reduce_lr_on_plateau", get_optimizer("nadam", None, lr=0.1), 10, factor=1.0, patience=0)
    fires = get_scheduler("reduce_lr_on_plateau", get_optimizer("nadam", None, lr=0.1), 10, factor=0.5, patience=8)
    assert not fires["constant_lr"] and fires["plateau"]["patience"] == 8
