"""CPU side of the detector-training tests (tests/test_gpu_training.py holds the device side): the networks, batches and clip
seeds both files run, the float64 specification (VariantDetector under torch autograd) with its float32 restatement, and a
mirror of the kernel choice det_plan makes for a training call (csrc/capi.hip, pipe = 1, readout = 1, training = true).

Checked here, without a GPU: every clip of the seed table keeps every LeakyReLU argument at least KINK from 0 in both
precisions (the one-pooled-frame clip is exactly 0 everywhere instead); the specification's parameter gradients agree with
central finite differences; the batch list reaches every alternative of the training plan; every network passes
training_refusal; every float32 floor the GPU tests take their bounds from is finite and below 1e-4."""
import functools

import numpy as np
import pytest
import torch

from conftest import make_clip
from test_detector_sizes_host import CARD, oracle_net
from test_detector_variants_host import VariantDetector

KINK = 8e-6            # the project's distance from a LeakyReLU kink (tests/loop_support.py)
FLOOR = 2e-5           # the least bound on a relative L2 distance or a loss (loop_support.check_gradient, test_gpu_seam.py)

NETWORKS = {
    "card": dict(),
    "blk0": dict(num_blocks=0, n_filters=[]),
    "w4_L1": dict(num_blocks=1, n_filters=[4], output_length=1),
    "w132_260": dict(num_blocks=2, n_filters=[132, 260]),
    "six128": dict(num_blocks=6, n_filters=[128] * 6),
    "w128_256": dict(num_blocks=2, n_filters=[128, 256]),
    "card_L64": dict(output_length=64),
    "card_L512": dict(output_length=512),
}
BATCHES = {
    "U31": [16000] * 3,
    "U64": [33000] * 2,
    "U97": [49700] * 2,
    "U128": [65280] * 2,
    "U129": [65792] * 2,
    "R": [16000, 24000, 600, 70000],
    "LONG": [165000, 16000],
    "ONE": [24000],
    "U31x4": [16000] * 4,          # the split-batch test's uniform case: twice [16000] * 2
    "U80": [41000] * 2,            # 80 pooled frames: three 32-row groups, the one group count the batches above leave out
}
CASES = [(net, b) for net in NETWORKS for b in ("U31", "R")] + [("card", b) for b in ("U64", "U80", "U97", "U128", "U129", "ONE")] + \
        [("w128_256", "LONG")]
ONE_FRAME = 600        # T = 3, one pooled frame: InstanceNorm over one frame gives exactly 0 in every block

# Clip seeds (conftest.make_clip) per (network, batch), one per clip.  Each was found by walking seeds upwards from 300 and
# keeping the first ones whose clip of that length keeps every block argument of that network at least KINK from 0 in the
# float64 and in the float32 restatement (kinks() below is the whole search).  The seeds tried and refused are in DESIGN.md
# section 34.  The 600-sample clip takes any seed.
SEEDS = {
    ("card", "U31"): [301, 303, 304],
    ("card", "R"): [301, 300, 300, 301],
    ("blk0", "U31"): [300, 301, 303],
    ("blk0", "R"): [300, 300, 300, 300],
    ("w4_L1", "U31"): [300, 301, 302],
    ("w4_L1", "R"): [300, 300, 300, 300],
    ("w132_260", "U31"): [300, 301, 303],
    ("w132_260", "R"): [300, 300, 300, 300],
    ("six128", "U31"): [300, 301, 303],
    ("six128", "R"): [300, 300, 300, 300],
    ("w128_256", "U31"): [300, 301, 303],
    ("w128_256", "R"): [300, 300, 300, 300],
    ("card_L64", "U31"): [301, 303, 304],
    ("card_L64", "R"): [301, 300, 300, 301],
    ("card_L512", "U31"): [301, 303, 304],
    ("card_L512", "R"): [301, 300, 300, 307],
    ("card", "U64"): [300, 303],
    ("card", "U80"): [307, 315],
    ("card", "U97"): [303, 306],
    ("card", "U128"): [303, 306],
    ("card", "U129"): [312, 323],
    ("card", "ONE"): [300],
    ("w128_256", "LONG"): [303, 300],
    ("card", "U31x4"): [301, 303, 304, 306],
}


def cfg(name):
    return dict(CARD, **NETWORKS[name])


def channels(name):
    c = cfg(name)
    return [c["n_mels"]] + list(c["n_filters"]) + [2 * c["output_length"]]


@functools.lru_cache(maxsize=None)
def network(name):
    return oracle_net(cfg(name))


@functools.lru_cache(maxsize=None)
def detector(name, dtype):
    return VariantDetector(network(name), dtype)


@functools.lru_cache(maxsize=None)
def band():
    from oracle import aware_oracle as O
    return O.band_indices()


@functools.lru_cache(maxsize=64)
def magnitude(seed, n):
    """|STFT(normalised clip)| in float32 with the bins outside the band zeroed, [1, 513, T]."""
    from oracle import aware_oracle as O
    a = torch.from_numpy(make_clip(seed, n)[0])[None]
    m = torch.abs(O.stft(a / torch.amax(torch.abs(a) + 1e-8))).clone()
    m[:, band()[1]] = 0.0
    return m


def kinks(name, seed, n):
    """The smallest |LeakyReLU argument| of the clip over all blocks, in the float64 and in the float32 restatement."""
    m = magnitude(seed, n)
    return float(detector(name, torch.float64).kink_distance(m.double())[0]), \
        float(detector(name, torch.float32).kink_distance(m)[0])


def per_clip_loss(loss, pred, target):
    """A loss of aware_amd/embedding/losses.py on one clip's prediction [L]."""
    from aware_amd.embedding.losses import get_loss_fn
    return get_loss_fn(loss).forward(pred, target)


def evaluate(name, lengths, seeds, dtype, cot=None, loss=None, target=None):
    """The specification at `dtype`: values [B, L], per-clip objective [B], dL/dW_l, dL/db_l and per-clip dL/dmag on the band
    rows ([225, T]) of the SUM over clips of the per-clip objective: sum(values * cot[i]) for an external cotangent, else the
    loss against target[i]."""
    det = VariantDetector(network(name), dtype)
    ws = [w.clone().requires_grad_(True) for w in det.ws]
    bs = [b.clone().requires_grad_(True) for b in det.bs]
    det.ws, det.bs = ws, bs
    mags, vals, objs = [], [], []
    for i, (s, n) in enumerate(zip(seeds, lengths)):
        m = magnitude(s, n).to(dtype).clone().requires_grad_(True)
        out = det.forward(m)[0]
        mags.append(m)
        vals.append(out.detach())
        objs.append((out * cot[i].to(dtype)).sum() if cot is not None else per_clip_loss(loss, out, target[i].to(dtype)).to(dtype))
    total = torch.stack(objs).sum()
    if total.requires_grad:
        total.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad            # noqa: E731  (ber: no gradient at all)
    return dict(values=torch.stack(vals), objective=torch.stack([o.detach() for o in objs]), dW=[zero(w) for w in ws],
                db=[zero(b) for b in bs], gmag=[zero(m)[0, band()[0]] for m in mags])


def rel(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-300))


def floors(r32, r64):
    """The float32 restatement's own distances from the float64 one: relative L2 per layer of dW, per clip of gmag, and the
    largest difference of a per-clip objective."""
    return dict(dW=[rel(a, b) for a, b in zip(r32["dW"], r64["dW"])],
                gmag=[rel(a, b) if float(b.norm()) > 0 else 0.0 for a, b in zip(r32["gmag"], r64["gmag"])],
                objective=float((r32["objective"].double() - r64["objective"]).abs().max()))


def cotangent(name, batch):
    L = cfg(name)["output_length"]
    g = torch.Generator().manual_seed(1000 + 17 * list(NETWORKS).index(name) + list(BATCHES).index(batch))
    return torch.randn(len(BATCHES[batch]), L, generator=g)


def bipolar(name, batch, seed=0):
    L = cfg(name)["output_length"]
    g = torch.Generator().manual_seed(2000 + seed + 17 * list(NETWORKS).index(name) + list(BATCHES).index(batch))
    return 2.0 * torch.randint(0, 2, (len(BATCHES[batch]), L), generator=g).float() - 1.0


@functools.lru_cache(maxsize=None)
def case_reference(name, batch):
    """(float64 evaluation, floors) of a case of CASES with its seeded external cotangent; computed once per process."""
    lengths, seeds, cot = BATCHES[batch], SEEDS[(name, batch)], cotangent(name, batch)
    r64 = evaluate(name, lengths, seeds, torch.float64, cot=cot)
    r32 = evaluate(name, lengths, seeds, torch.float32, cot=cot)
    return r64, floors(r32, r64)


def reference_training(name, lengths, seeds, target, dtype, steps=3, lr=1e-3):
    """`steps` steps of torch.optim.Adam on the specification at `dtype` with the objective of aware_amd/training.py (mean over
    the clips of mse - 0.1 mean|raw|): the losses and the weights after the last step."""
    det = VariantDetector(network(name), dtype)
    ws = [w.clone().requires_grad_(True) for w in det.ws]
    bs = [b.clone().requires_grad_(True) for b in det.bs]
    det.ws, det.bs = ws, bs
    adam = torch.optim.Adam(ws + bs, lr=lr)
    mags = [magnitude(s, n).to(dtype) for s, n in zip(seeds, lengths)]
    losses = []
    for _ in range(steps):
        adam.zero_grad()
        loss = torch.stack([per_clip_loss("push_extremes", det.forward(m)[0], target[i].to(dtype)) for i, m in enumerate(mags)]).mean()
        loss.backward()
        adam.step()
        losses.append(float(loss))
    return losses, [w.detach().clone() for w in ws]


LOSSES = ["push_extremes", "mse", "hinge", "sign", "push_sigmoid", "ber"]           # loss_kind 0..5
LOSS_BATCHES = ["U31", "R"]


@functools.lru_cache(maxsize=None)
def loss_reference(batch, loss):
    """(float64 evaluation, floors) of the card's network on `batch` with `loss` inside against seeded bipolar targets."""
    lengths, seeds, target = BATCHES[batch], SEEDS[("card", batch)], bipolar("card", batch)
    r64 = evaluate("card", lengths, seeds, torch.float64, loss=loss, target=target)
    r32 = evaluate("card", lengths, seeds, torch.float32, loss=loss, target=target)
    return r64, floors(r32, r64)


TRAINER_CASES = [("card", "U31"), ("w132_260", "R")]


@functools.lru_cache(maxsize=None)
def trainer_reference(name, batch):
    """(float64 losses, float64 weights, loss floor, per-layer weight floors) of three Adam steps at lr = 1e-3."""
    lengths, seeds, target = BATCHES[batch], SEEDS[(name, batch)], bipolar(name, batch, seed=7)
    l64, w64 = reference_training(name, lengths, seeds, target, torch.float64)
    l32, w32 = reference_training(name, lengths, seeds, target, torch.float32)
    return l64, w64, float(np.abs(np.asarray(l32) - np.asarray(l64)).max()), [rel(a, b) for a, b in zip(w32, w64)]


# ---- the mirror of det_plan for a training call -------------------------------------------------------------------------------
MEL_CLIP_FRAMES = 192      # kMelClipFrames (csrc/kernels.h)
TAIL_MAX_POOLED = 320      # the split-K last block and launch_tail serve max_frames / 2 <= 320


def training_plan(chans, lengths):
    """What det_plan(d, b, pipe = 1, readout = 1, training = true) chooses for a network of the caller's `chans` on clips of
    `lengths` samples: per block the forward kind ("splitk" for the last block under the tail, else "clip" / "plain") and the
    data-gradient kind ("clip" / "plain"), whether a clip launch runs the aligned template of launch_gemm_clip (K % 32 == 0
    and N % 128 == 0), whether the block's weight gradient reads a dL/dZ written by a fused epilogue (dz), the read-out, and
    the form of the mel stage."""
    from aware_amd.runtime import stored_channels
    ch = stored_channels(chans)
    nl = len(ch) - 1
    frames = [1 + n // 256 for n in lengths]
    pooled = [t // 2 for t in frames]
    uniform_tp = pooled[0] if all(p == pooled[0] for p in pooled) else 0
    groups = (uniform_tp + 31) // 32
    nwm = groups if uniform_tp and 1 <= groups <= 4 else 0
    fwd, bwd, dz, aligned = [], [None] * nl, [None] * nl, []
    for l in range(nl):
        ci, co = ch[l], ch[l + 1]
        if l == nl - 1 and co <= 64 and max(frames) // 2 <= TAIL_MAX_POOLED:
            fwd.append("splitk")
        elif nwm and co >= 128:
            fwd.append("clip")
            aligned.append(("fwd", l, ci % 32 == 0 and co % 128 == 0))
        else:
            fwd.append("plain")
    readout = "tail" if fwd[-1] == "splitk" else "wide" if ch[nl] > 64 else "head"
    for l in range(nl - 1, -1, -1):
        ci, co = ch[l], ch[l + 1]
        dz[l] = readout != "head" if l == nl - 1 else bwd[l + 1] != "plain"
        if nwm and l > 0 and ci >= 128:
            bwd[l] = "clip"
            aligned.append(("bwd", l, co % 32 == 0 and ci % 128 == 0))
        else:
            bwd[l] = "plain"
    return dict(n_layers=nl, uniform=bool(uniform_tp), nwm=nwm, fwd=fwd, bwd=bwd, dz=dz, aligned=aligned, readout=readout,
                mel="chunked" if max(frames) > MEL_CLIP_FRAMES else "clip", contraction=sum((p + 31) // 32 * 32 for p in pooled))


# ---- tests --------------------------------------------------------------------------------------------------------------------
def test_every_case_has_seeds():
    assert set(SEEDS) == set(CASES) | {("card", "U31x4")}
    for (name, batch), seeds in SEEDS.items():
        assert len(seeds) == len(BATCHES[batch]), (name, batch)
        assert len(set(zip(seeds, BATCHES[batch]))) == len(seeds), (name, batch)       # no clip twice in a batch


@pytest.mark.parametrize("name,batch", list(SEEDS) if SEEDS else CASES)
def test_seed_table_keeps_clear_of_the_kinks(name, batch):
    """Every clip of the table: every block argument at least KINK from 0 in float64 and in float32.  The 600-sample clip:
    every block argument exactly 0 in both precisions, and with it dL/dZ: it adds exactly nothing to any dW, db."""
    for seed, n in zip(SEEDS[(name, batch)], BATCHES[batch]):
        if n == ONE_FRAME:
            for dtype in (torch.float64, torch.float32):
                m = magnitude(seed, n).to(dtype)
                us = detector(name, dtype).pre_activations(m)
                assert m.shape[-1] == 3 and all(u.shape[-1] == 1 for u in us[:-1])
                assert all(float(u.abs().max()) == 0.0 for u in us), (name, dtype)
            continue
        k64, k32 = kinks(name, seed, n)
        assert min(k64, k32) >= KINK, (name, batch, seed, n, k64, k32)


@pytest.mark.parametrize("name", list(NETWORKS))
def test_one_frame_clip_adds_nothing_to_the_parameter_gradients(name):
    """The reference on the 600-sample clip alone, any cotangent: dL/dW and dL/db are exactly 0 (its dL/dmag is not asked)."""
    cot = torch.randn(1, cfg(name)["output_length"], generator=torch.Generator().manual_seed(4))
    for dtype in (torch.float64, torch.float32):
        r = evaluate(name, [ONE_FRAME], [300], dtype, cot=cot)
        assert float(r["values"].abs().max()) == 0.0
        for g in r["dW"] + r["db"]:
            assert float(g.abs().max()) == 0.0 and bool(torch.isfinite(g).all())


@pytest.mark.parametrize("name", ["w4_L1", "blk0"])
def test_specification_agrees_with_finite_differences(name):
    """float64 autograd dW / db of the specification against central differences at step 1e-6, on a two-clip batch: relative
    L2 per tensor (absolute for a gradient that is 0 up to rounding: the bias behind an InstanceNorm) below 1e-6.  Sampled:
    every entry of the small tensors, 64 seeded entries of the large ones."""
    lengths, seeds = [16000, 24000], [300, 301]
    cot = torch.randn(2, cfg(name)["output_length"], generator=torch.Generator().manual_seed(8))
    r = evaluate(name, lengths, seeds, torch.float64, cot=cot)
    det = VariantDetector(network(name), torch.float64)
    mags = [magnitude(s, n).double() for s, n in zip(seeds, lengths)]

    def objective():
        with torch.no_grad():
            return float(sum((det.forward(m)[0] * cot[i].double()).sum() for i, m in enumerate(mags)))

    rng = np.random.default_rng(5)
    h = 1e-6
    scale = max(float(g.abs().max()) for g in r["dW"])
    for kind, params, grads in (("dW", det.ws, r["dW"]), ("db", det.bs, r["db"])):
        for l, (p, g) in enumerate(zip(params, grads)):
            flat = p.view(-1)
            idx = np.arange(flat.numel()) if flat.numel() <= 64 else rng.choice(flat.numel(), 64, replace=False)
            fd = np.zeros(len(idx))
            for j, k in enumerate(idx):
                keep = float(flat[k])
                flat[k] = keep + h
                up = objective()
                flat[k] = keep - h
                down = objective()
                flat[k] = keep
                fd[j] = (up - down) / (2 * h)
            an = g.reshape(-1)[idx].numpy()
            err = float(np.linalg.norm(fd - an)) / max(float(np.linalg.norm(an)), scale * np.sqrt(len(idx)) * 1e-3)
            print(f"{name} {kind}[{l}]: central differences vs autograd {err:.2e} (|autograd| {np.linalg.norm(an):.2e})")
            assert err < 1e-6, (name, kind, l, err)


def test_every_network_is_served():
    from aware_amd import runtime as rt
    for name in NETWORKS:
        assert rt.training_refusal(channels(name)) is None, name
        assert channels(name)[0] == 128


def test_batches_have_the_frames_they_are_named_for():
    pooled = {k: [(1 + n // 256) // 2 for n in v] for k, v in BATCHES.items()}
    assert pooled["U31"] == [31] * 3 and pooled["U64"] == [64] * 2 and pooled["U80"] == [80] * 2 and pooled["U97"] == [97] * 2
    assert pooled["U128"] == [128] * 2 and pooled["U129"] == [129] * 2
    assert 1 + 49700 // 256 == 195 and pooled["R"] == [31, 47, 1, 137] and pooled["LONG"] == [322, 31]
    assert all(n <= 165000 for v in BATCHES.values() for n in v) and all(len(v) <= 4 for v in BATCHES.values())


def test_batch_list_reaches_every_alternative_of_the_training_plan():
    plans = {(n, b): training_plan(channels(n), BATCHES[b]) for n, b in CASES}
    hit = lambda pred: [k for k, p in plans.items() if pred(p)]                 # noqa: E731
    clip_aligned = hit(lambda p: any(a for _, _, a in p["aligned"]))
    clip_unaligned = hit(lambda p: any(not a for _, _, a in p["aligned"]))
    assert ("card", "U31") in clip_aligned and ("card", "U128") in clip_aligned
    assert ("w132_260", "U31") in clip_unaligned
    # both directions of the unaligned template: forward (K = 132, N = 260) and data gradient (K = 260, N = 132)
    assert {d for d, _, a in plans[("w132_260", "U31")]["aligned"] if not a} == {"fwd", "bwd"}
    # the benchmark's path: the weight gradient of a block reads dL/dZ from the fused backward epilogue above it
    assert plans[("card", "U31")]["dz"] == [True, True, True, True] and plans[("card", "U31")]["bwd"] == ["plain", "clip", "clip", "clip"]
    assert hit(lambda p: p["uniform"] and not p["nwm"]) == [("card", "U129")]          # plain on a uniform batch
    assert all(k == "plain" for k in plans[("card", "U129")]["fwd"][:-1] + plans[("card", "U129")]["bwd"])
    assert ("card", "R") in hit(lambda p: not p["uniform"] and "clip" not in p["fwd"] + p["bwd"])     # plain on a ragged batch
    assert plans[("w4_L1", "U31")]["fwd"] == ["plain", "splitk"] and plans[("w4_L1", "U31")]["bwd"] == ["plain", "plain"]
    assert {p["readout"] for p in plans.values()} == {"tail", "head", "wide"}
    assert hit(lambda p: p["readout"] == "head") == [("w128_256", "LONG")]
    assert plans[("w128_256", "LONG")]["fwd"][-1] == "plain" and plans[("w128_256", "LONG")]["dz"][-1] is False
    assert set(hit(lambda p: p["readout"] == "wide")) == {(n, b) for n in ("card_L64", "card_L512") for b in ("U31", "R")}
    assert plans[("card_L64", "U31")]["fwd"][-1] == "clip" and plans[("card_L64", "R")]["fwd"][-1] == "plain"
    assert {p["mel"] for p in plans.values()} == {"clip", "chunked"}
    assert plans[("card", "U97")]["mel"] == "chunked" and plans[("card", "U64")]["mel"] == "clip" and plans[("card", "R")]["mel"] == "chunked"
    assert {p["n_layers"] for p in plans.values()} >= {1, 7}
    assert plans[("blk0", "U31")]["n_layers"] == 1 and plans[("six128", "R")]["n_layers"] == 7
    assert {p["nwm"] for p in plans.values()} == {0, 1, 2, 3, 4}                  # 31, 64, 80, 97 / 128 pooled rows; none
    # the contraction length of dW = dZ^T X: the pooled rows with every clip's padding to 32
    assert {plans[("card", b)]["contraction"] for b in ("U31", "U64", "U80", "U97", "U128", "U129", "R", "ONE")} == \
        {96, 128, 192, 256, 320, 32 + 64 + 32 + 160, 64}
    # a batch of one is uniform, whatever its length
    assert plans[("card", "ONE")]["uniform"] and plans[("card", "ONE")]["nwm"] == 2


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("batch", LOSS_BATCHES)
def test_loss_floors_are_small(batch, loss):
    """The floors of the GPU test of the losses inside: per-clip loss and dW in float32 against float64, finite and below 1e-4;
    ber has no gradient in either precision."""
    r64, fl = loss_reference(batch, loss)
    worst = max(fl["dW"] + [fl["objective"]])
    assert np.isfinite(worst) and worst < 1e-4, (batch, loss, fl)
    assert bool(torch.isfinite(r64["objective"]).all())
    if loss == "ber":
        assert all(float(g.abs().max()) == 0.0 for g in r64["dW"] + r64["db"])
    else:
        assert all(float(g.norm()) > 0 for g in r64["dW"])


@pytest.mark.parametrize("name,batch", TRAINER_CASES)
def test_trainer_floors_are_small(name, batch):
    """Three Adam steps in float32 against float64: the floors of the trainer test are finite and below 1e-4, and the steps
    reduce the loss of their own batch."""
    l64, _, lfloor, wfloors = trainer_reference(name, batch)
    print(f"{name} {batch}: losses {l64}, float32 floors: loss {lfloor:.1e}, weights {['%.1e' % v for v in wfloors]}")
    assert np.isfinite(lfloor) and lfloor < 1e-4 and all(np.isfinite(v) and v < 1e-4 for v in wfloors)
    assert l64[2] < l64[0]


@pytest.mark.parametrize("name,batch", list(SEEDS) if SEEDS else CASES)
def test_float32_floors_are_small(name, batch):
    """Every float32 floor the GPU tests multiply by four is finite and below 1e-4 on the chosen seeds."""
    _, fl = case_reference(name, batch)
    worst = max(fl["dW"] + fl["gmag"] + [fl["objective"]])
    print(f"{name} {batch}: float32 floors dW {['%.1e' % v for v in fl['dW']]} gmag {['%.1e' % v for v in fl['gmag']]}")
    assert np.isfinite(worst) and worst < 1e-4, (name, batch, fl)
