"""GPU tests of the detector-training extension (aware_detector_weight_gradients, aware_detector_train_gradients,
aware_detector_update / _update_device, DetectorTrainer) on every network, batch and loss it serves, against the float64
specification of tests/test_training_host.py (VariantDetector under torch autograd on the oracle's network).

The cases, their clip seeds and the alternatives of the training plan each one reaches are in test_training_host.py, which
checks on the CPU that no clip comes within KINK of a LeakyReLU kink in either precision.  Bounds: the figures other tests of
this repository hold (5e-5 for values, 1e-4 * max|dW| * Cin for the bias gradients that vanish behind an InstanceNorm) and,
for every relative L2 distance and every loss, four times the distance of the float32 restatement from the float64 one,
computed here on the CPU, and at least 2e-5.  Where the code promises equal bits (optional pointers, repeated calls, the
rebuilt device images of the parameters) equality is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_training_host as H
from conftest import make_clip

pytestmark = pytest.mark.gpu

VALUES_ATOL = 5e-5


@pytest.fixture(scope="module")
def rt():
    from aware_amd import runtime
    from aware_amd._lib import require_gpu
    require_gpu()
    return runtime


@pytest.fixture(scope="module")
def plan(rt):
    from aware_amd.utils.audio import default_plan
    return default_plan()


def new_net(name):
    from aware_amd.detection import AWAREDetectorNet
    c = H.cfg(name)
    return AWAREDetectorNet(n_mels=c["n_mels"], num_blocks=c["num_blocks"], n_filters=c["n_filters"],
                            output_length=c["output_length"])


_NETS = {}


def device_net(name):
    """The network of `name` with its seeded weights; shared by the tests that do not change them."""
    if name not in _NETS:
        _NETS[name] = new_net(name)
    return _NETS[name]


def inputs(rt, plan, lengths, seeds):
    clips = [make_clip(s, n)[0] for s, n in zip(seeds, lengths)]
    batch = rt.Batch(lengths)
    x = batch.pack(clips)
    mag, _ = rt.stft_band(plan, batch, x, normalize=True)
    return batch, x, mag


def train_call(rt, plan, dev, batch, mag, target, loss=None, skip_w=(), skip_b=(), biases=True, values=True, gmag=True):
    """aware_detector_weight_gradients (loss None: `target` is the cotangent) or aware_detector_train_gradients through the C
    ABI with any of the optional pointers NULL.  Every output buffer starts as NaN; a skipped one is allocated, poisoned and
    its pointer nulled, and comes back as it was."""
    lib, dv = plan.lib, mag.device
    nan = float("nan")
    nbytes = lib.aware_detector_train_workspace_bytes(batch.h, dev.h)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dv)
    ch = dev.channels
    nl = len(ch) - 1
    out = dict(values=torch.full((batch.B, dev.n_bits), nan, device=dv), losses=torch.full((batch.B,), nan, device=dv),
               gmag=torch.full((batch.total_frames, plan.band_stride), nan, device=dv),
               dW=[torch.full((ch[i + 1], ch[i]), nan, device=dv) for i in range(nl)],
               db=[torch.full((ch[i + 1],), nan, device=dv) for i in range(nl)])
    pw = (C.c_void_p * nl)(*[None if i in skip_w else out["dW"][i].data_ptr() for i in range(nl)])
    pb = (C.c_void_p * nl)(*[None if i in skip_b else out["db"][i].data_ptr() for i in range(nl)]) if biases else None
    tg = target.to(dv).contiguous().float()
    pv = rt._ptr(out["values"]) if values else None
    pg = rt._ptr(out["gmag"]) if gmag else None
    if loss is None:
        rt.check(lib.aware_detector_weight_gradients(dev.h, batch.h, rt._ptr(mag), rt._ptr(tg), pv, pg, pw, pb, rt._ptr(ws), nbytes,
                                                     rt._stream()), "aware_detector_weight_gradients")
    else:
        rt.check(lib.aware_detector_train_gradients(dev.h, batch.h, rt._ptr(mag), rt._ptr(tg), rt.LOSS_KINDS[loss],
                                                    rt._ptr(out["losses"]), pv, pg, pw, pb, rt._ptr(ws), nbytes, rt._stream()),
                 "aware_detector_train_gradients")
    torch.cuda.synchronize()
    return out


def bound(floor, scale=1.0):
    return scale * max(4 * floor, H.FLOOR)


def check_case(tag, rt, batch, out, r64, fl, scale=1.0, gmag=True):
    """values, dW, db and grad_mag of a device call (dict of train_call, device tensors) against the float64 evaluation r64
    with the float32 floors fl; `scale` multiplies every bound (the split-batch test allows twice)."""
    vals = out["values"].cpu().numpy()
    verr = float(np.abs(vals - r64["values"].numpy()).max())
    print(f"{tag}: values max err {verr:.1e} (bound {VALUES_ATOL:.0e})")
    assert verr <= VALUES_ATOL, (tag, verr)
    for l, (w, b, ref, bref) in enumerate(zip(out["dW"], out["db"], r64["dW"], r64["db"])):
        assert tuple(w.shape) == tuple(ref.shape) and tuple(b.shape) == tuple(bref.shape), (tag, l, w.shape, ref.shape)
        err, bnd = H.rel(w.cpu(), ref), bound(fl["dW"][l], scale)
        berr, bbnd = float(b.abs().max()), scale * 1e-4 * float(ref.abs().max()) * ref.shape[1]
        print(f"{tag} layer {l}: dL/dW rel L2 {err:.2e} (float32 restatement {fl['dW'][l]:.1e}, bound {bnd:.1e}); "
              f"|dL/db| max {berr:.1e} (bound {bbnd:.1e}, float64 autograd {float(bref.abs().max()):.1e})")
        assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(b).all()), (tag, l)
        assert err <= bnd, (tag, l, err, bnd)
        assert berr < bbnd, (tag, l, berr, bbnd)
    if not gmag:
        return
    g = out["gmag"].cpu()
    assert bool(torch.isfinite(g).all()), tag
    assert float(g[:, 225:].abs().max()) == 0.0, tag                                 # the padding columns of the band layout
    fo = batch.frame_offsets
    for i, ref in enumerate(r64["gmag"]):
        mine = g[fo[i]: fo[i + 1], :225].T
        if float(ref.norm()) == 0.0:                                                 # the one-pooled-frame clip: dL/dZ is exactly 0
            assert float(mine.abs().max()) == 0.0, (tag, i)
            continue
        err, bnd = H.rel(mine, ref), bound(fl["gmag"][i], scale)
        print(f"{tag} clip {i}: grad_mag rel L2 {err:.2e} (float32 restatement {fl['gmag'][i]:.1e}, bound {bnd:.1e})")
        assert err <= bnd, (tag, i, err, bnd)


# ---- 1. weight gradients, external cotangent ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,batch", H.CASES)
def test_weight_gradients_external_cotangent(rt, plan, name, batch):
    """rt.detector_weight_gradients on every (network, batch) of the training plan against float64 autograd of the sum over
    the clips: values, dL/dW and dL/db per layer in the caller's shapes ([2L][Cin] and [2L] for the last), grad_mag per clip."""
    r64, fl = H.case_reference(name, batch)
    dev = device_net(name).device_weights(plan)
    b, _, mag = inputs(rt, plan, H.BATCHES[batch], H.SEEDS[(name, batch)])
    vals, gmag, gw, gb = rt.detector_weight_gradients(plan, dev, b, mag, H.cotangent(name, batch).cuda())
    torch.cuda.synchronize()
    L, ch = H.cfg(name)["output_length"], H.channels(name)
    assert tuple(gw[-1].shape) == (2 * L, ch[-2]) and tuple(gb[-1].shape) == (2 * L,)
    p = H.training_plan(ch, H.BATCHES[batch])
    print(f"{name} {batch}: forward {p['fwd']}, data gradient {p['bwd']}, read-out {p['readout']}, mel {p['mel']}, K = {p['contraction']}")
    check_case(f"{name} {batch}", rt, b, dict(values=vals, gmag=gmag, dW=gw, db=gb), r64, fl)


# ---- 2. losses inside ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", H.LOSSES)
@pytest.mark.parametrize("batch", H.LOSS_BATCHES)
def test_train_gradients_every_loss(rt, plan, batch, loss):
    """rt.detector_train_gradients on the card's network for every loss 0..5 with bipolar targets: the per-clip losses, and
    dW / db of their sum, against the float64 evaluation of aware_amd/embedding/losses.py; ber has no gradient at all."""
    r64, fl = H.loss_reference(batch, loss)
    dev = device_net("card").device_weights(plan)
    b, _, mag = inputs(rt, plan, H.BATCHES[batch], H.SEEDS[("card", batch)])
    vals, losses, gw, gb = rt.detector_train_gradients(plan, dev, b, mag, H.bipolar("card", batch).cuda(), loss)
    torch.cuda.synchronize()
    lerr = float((losses.cpu().double() - r64["objective"]).abs().max())
    lbound = bound(fl["objective"])
    print(f"card {batch} {loss}: per-clip loss max err {lerr:.1e} (float32 restatement {fl['objective']:.1e}, bound {lbound:.1e})")
    assert lerr <= lbound, (loss, lerr, lbound)
    if loss == "ber":
        np.testing.assert_allclose(vals.cpu().numpy(), r64["values"].numpy(), atol=VALUES_ATOL)
        for g in gw + gb:
            assert bool(torch.isfinite(g).all()) and float(g.abs().max()) == 0.0
        return
    check_case(f"card {batch} {loss}", rt, b, dict(values=vals, dW=gw, db=gb), r64, fl, gmag=False)


def test_train_gradients_refuses_the_l1_loss(rt, plan):
    """push_extremes_l1 needs the embed loop's coefficients: a bad argument, not push_extremes in its place."""
    from aware_amd._lib import AwareHipError
    dev = device_net("card").device_weights(plan)
    b, _, mag = inputs(rt, plan, H.BATCHES["U31"], H.SEEDS[("card", "U31")])
    with pytest.raises(AwareHipError, match="bad argument"):
        rt.detector_train_gradients(plan, dev, b, mag, H.bipolar("card", "U31").cuda(), "push_extremes_l1")


# ---- 3. optional pointers -----------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def untouched(t):
    return bool(torch.isnan(t).all())


@pytest.mark.parametrize("batch", ["U31", "R"])
def test_optional_pointers(rt, plan, batch):
    """grad_weights[l] NULL for some layers, grad_biases[l] NULL for others, grad_biases NULL, values NULL, grad_mag NULL: what
    is still asked for has the bits of the full call, and a buffer whose pointer was nulled is not written."""
    dev = device_net("card").device_weights(plan)
    b, _, mag = inputs(rt, plan, H.BATCHES[batch], H.SEEDS[("card", batch)])
    tg = H.bipolar("card", batch)
    full = train_call(rt, plan, dev, b, mag, tg, "push_extremes")
    for k in ("values", "losses", "gmag"):
        assert bool(torch.isfinite(full[k]).all())
    assert all(bool(torch.isfinite(t).all()) for t in full["dW"] + full["db"])

    def agree(got, asked_w, asked_b, values=True, gmag=True):
        assert same_bits(got["losses"], full["losses"])
        assert same_bits(got["values"], full["values"]) if values else untouched(got["values"])
        assert same_bits(got["gmag"], full["gmag"]) if gmag else untouched(got["gmag"])
        for l in range(4):
            assert same_bits(got["dW"][l], full["dW"][l]) if l in asked_w else untouched(got["dW"][l]), ("dW", l)
            assert same_bits(got["db"][l], full["db"][l]) if l in asked_b else untouched(got["db"][l]), ("db", l)

    every = (0, 1, 2, 3)
    # a bias gradient is written whether or not the weight gradient of its layer is asked for, and the other way round
    agree(train_call(rt, plan, dev, b, mag, tg, "push_extremes", skip_w=(0, 2)), (1, 3), every)
    agree(train_call(rt, plan, dev, b, mag, tg, "push_extremes", skip_w=(1, 3), skip_b=(0, 3)), (0, 2), (1, 2))
    agree(train_call(rt, plan, dev, b, mag, tg, "push_extremes", biases=False), every, ())
    agree(train_call(rt, plan, dev, b, mag, tg, "push_extremes", values=False), every, every, values=False)
    agree(train_call(rt, plan, dev, b, mag, tg, "push_extremes", gmag=False, skip_w=every, skip_b=(0, 1, 2)), (), (3,), gmag=False)
    # the external-cotangent entry point takes the same optional pointers (values may be NULL, grad_mag may not)
    cot = H.cotangent("card", batch)
    full = train_call(rt, plan, dev, b, mag, cot)
    got = train_call(rt, plan, dev, b, mag, cot, skip_w=(3,), skip_b=(0,), values=False)
    assert same_bits(got["gmag"], full["gmag"]) and untouched(got["values"])
    for l in range(4):
        assert same_bits(got["dW"][l], full["dW"][l]) if l != 3 else untouched(got["dW"][l])
        assert same_bits(got["db"][l], full["db"][l]) if l != 0 else untouched(got["db"][l])


# ---- 4. sum over a split batch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,cut", [("R", 2), ("U31x4", 2)])
def test_gradients_add_up_over_a_split_batch(rt, plan, batch, cut):
    """What the all-reduce rests on: dW, db of a batch are the sums of those of its two halves run as two batches (R: both
    halves ragged, the plain path on both sides; four 1 s clips: the clip kernels on both sides).  The summed halves are held
    to the float64 evaluation of the whole batch with twice the bound of the whole batch."""
    r64, fl = H.case_reference("card", batch)
    dev = device_net("card").device_weights(plan)
    lengths, seeds, cot = H.BATCHES[batch], H.SEEDS[("card", batch)], H.cotangent("card", batch)
    for part in (lengths, lengths[:cut], lengths[cut:]):
        kinds = H.training_plan(H.channels("card"), part)
        assert ("clip" in kinds["bwd"]) == (batch == "U31x4")
    halves = []
    for sl in (slice(0, cut), slice(cut, None)):
        b, _, mag = inputs(rt, plan, lengths[sl], seeds[sl])
        halves.append((b, train_call(rt, plan, dev, b, mag, cot[sl])))
    total = dict(values=torch.cat([h["values"] for _, h in halves]), dW=[x + y for x, y in zip(halves[0][1]["dW"], halves[1][1]["dW"])],
                 db=[x + y for x, y in zip(halves[0][1]["db"], halves[1][1]["db"])])
    check_case(f"card {batch} as two batches", rt, None, total, r64, fl, scale=2.0, gmag=False)
    b, _, mag = inputs(rt, plan, lengths, seeds)
    whole = train_call(rt, plan, dev, b, mag, cot)
    for l in range(4):
        print(f"card {batch} layer {l}: whole batch vs summed halves rel L2 {H.rel(total['dW'][l].cpu(), whole['dW'][l].cpu()):.2e}")
    # a clip's values and grad_mag do not depend on its neighbours' lengths beyond rounding: each half against its clips
    fo = 0
    for (hb, h), sl in zip(halves, (slice(0, cut), slice(cut, None))):
        part = dict(r64, gmag=r64["gmag"][sl])
        g = h["gmag"].cpu()
        for i, ref in enumerate(part["gmag"]):
            mine = g[hb.frame_offsets[i]: hb.frame_offsets[i + 1], :225].T
            if float(ref.norm()) == 0.0:
                assert float(mine.abs().max()) == 0.0
            else:
                assert H.rel(mine, ref) <= bound(fl["gmag"][fo + i])
        fo += len(part["gmag"])


# ---- 5. repeatability ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", ["U31", "R"])
def test_two_calls_give_the_same_bits(rt, plan, batch):
    dev = device_net("card").device_weights(plan)
    b, _, mag = inputs(rt, plan, H.BATCHES[batch], H.SEEDS[("card", batch)])
    for target, loss in ((H.bipolar("card", batch), "push_extremes"), (H.cotangent("card", batch), None)):
        one = train_call(rt, plan, dev, b, mag, target, loss)
        two = train_call(rt, plan, dev, b, mag, target, loss)
        assert same_bits(one["values"], two["values"]) and same_bits(one["gmag"], two["gmag"])
        assert loss is None or same_bits(one["losses"], two["losses"])
        for l in range(4):
            assert same_bits(one["dW"][l], two["dW"][l]) and same_bits(one["db"][l], two["db"][l]), (loss, l)
        assert bool(torch.isfinite(one["gmag"]).all())


# ---- 6. the refreshed detector, every image -----------------------------------------------------------------------------------
DETECT_BATCHES = [[16000] * 3, [16000, 24000]]


def detector_outputs(rt, plan, dev, tag):
    """Everything that reads a device image of the parameters, as a dict of host arrays: aware_detect (the default pipe),
    aware_detector_backward, and the embed loop's first iteration on the f32, bf16 three-term and f16 two-term pipes with the
    fused and the three-kernel read-out -- w, wT, wpk, wTpk, wh2, wTh2, lastpk, lastTpk and the biases between them."""
    out = {}
    for lengths in DETECT_BATCHES:
        key = f"{tag} {lengths}"
        clips = [make_clip(400 + i, n)[0] for i, n in enumerate(lengths)]
        batch = rt.Batch(lengths)
        x = batch.pack(clips)
        gen = torch.Generator().manual_seed(len(lengths))
        gv = torch.randn(len(lengths), dev.n_bits, generator=gen).cuda()
        wm = (2.0 * torch.randint(0, 2, (len(lengths), dev.n_bits), generator=gen).float() - 1.0).cuda()
        out[f"{key} detect"] = rt.detect(plan, dev, batch, x).cpu().numpy()
        mag, _ = rt.stft_band(plan, batch, x, normalize=True)
        vals, gmag = rt.detector_backward(plan, dev, batch, mag, gv)
        out[f"{key} backward values"], out[f"{key} backward grad_mag"] = vals.cpu().numpy(), gmag.cpu().numpy()
        uniform = len(set(lengths)) == 1
        for pipe in ("f32", "bf16x3", "f16x2"):
            for fused in ((True, False) if uniform else (True,)):
                sess = rt.EmbedSession(plan, dev, batch, use_graph=False, conv_pipe=pipe, fused_readout=fused)
                sess.begin(x, wm)
                g = sess.gradient().cpu().numpy()
                k = f"{key} embed {pipe} fused_readout={fused}"
                out[f"{k} gradient"], out[f"{k} loss"], out[f"{k} pred"] = g, sess.loss.cpu().numpy().copy(), sess.pred.cpu().numpy().copy()
                del sess
    torch.cuda.synchronize()
    return out


def assert_same_detector(rt, plan, a, b, tag):
    """Device detectors a and b give the same bits wherever an image of the parameters is read."""
    oa, ob = detector_outputs(rt, plan, a, tag), detector_outputs(rt, plan, b, tag)
    differ = []
    for k in oa:
        assert np.isfinite(oa[k]).all(), k
        if not np.array_equal(oa[k].view(np.int32), ob[k].view(np.int32)):
            differ.append((k, float(np.abs(oa[k] - ob[k]).max())))
    assert not differ, differ


def perturbed(net, seed):
    """Every weight and bias of the network with seeded noise of relative size 1e-2 (the zero biases: of the size of 1e-2 of
    the layer's weights)."""
    rng = np.random.default_rng(seed)
    ws = [(w * (1 + 1e-2 * rng.standard_normal(w.shape))).astype(np.float32) for w in net.weights]
    bs = [(b + 1e-2 * float(np.abs(w).mean()) * rng.standard_normal(b.shape)).astype(np.float32) for w, b in zip(net.weights, net.biases)]
    return ws, bs


@pytest.mark.parametrize("how", ["device", "host", "device, biases NULL"])
@pytest.mark.parametrize("name", ["card", "w132_260"])
def test_refreshed_detector_is_the_fresh_one(rt, plan, name, how):
    """aware_detector_update_device (device tensors; also with dev_biases NULL: biases unchanged, weights new) and
    aware_detector_update (host arrays) leave every device image of the parameters as aware_detector_create builds it from
    the same numbers: x3_pack on the host and x3_pack_dev_kernel on the device state the same three-term split, and
    launch_h2_pack builds the f16 images on both sides."""
    net = new_net(name)
    w0, b0 = perturbed(net, 1)
    w1, b1 = perturbed(net, 2)
    dev = rt.DetectorWeights(plan, net.mel_basis, w0, b0)
    if how == "host":
        dev.update(w1, b1)
    elif how == "device":
        dev.update_device([torch.from_numpy(w).cuda() for w in w1], [torch.from_numpy(b).cuda() for b in b1])
    else:
        keep = [torch.from_numpy(w).cuda() for w in w1]
        pw = (C.c_void_p * len(keep))(*[t.data_ptr() for t in keep])
        rt.check(dev.lib.aware_detector_update_device(dev.h, pw, None, rt._stream()), "aware_detector_update_device")
        b1 = b0
    torch.cuda.synchronize()
    fresh = rt.DetectorWeights(plan, net.mel_basis, w1, b1)
    assert_same_detector(rt, plan, dev, fresh, f"{name} {how}")
    # and the refresh did change what the detector computes
    stale = rt.DetectorWeights(plan, net.mel_basis, w0, b0)
    batch = rt.Batch(DETECT_BATCHES[0])
    x = batch.pack([make_clip(400 + i, n)[0] for i, n in enumerate(DETECT_BATCHES[0])])
    assert not torch.equal(rt.detect(plan, stale, batch, x), rt.detect(plan, dev, batch, x))


# ---- 7. the trainer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,batch", H.TRAINER_CASES)
def test_trainer_three_steps(rt, name, batch):
    """DetectorTrainer.step three times at lr = 1e-3 against torch.optim.Adam on the float64 specification with the objective
    of training.py: losses and weights within four times the distance of the same steps in float32 (at least 2e-5), the loss
    falls, and after sync_host() the trained device copy is the detector a fresh upload of the host copy gives.  (The biases
    are not compared: their gradient is rounding noise behind the InstanceNorm, which Adam normalises to steps of its own.)"""
    from aware_amd.detection import AWAREDetector
    from aware_amd.training import DetectorTrainer
    l64, w64, lfloor, wfloors = H.trainer_reference(name, batch)
    lengths, seeds = H.BATCHES[batch], H.SEEDS[(name, batch)]
    net = new_net(name)
    before = [w.copy() for w in net.weights]
    det = AWAREDetector(model=net)
    plan = det._plan(16000)
    b, x, _ = inputs(rt, plan, lengths, seeds)
    bits = ((H.bipolar(name, batch, seed=7) + 1) / 2).to(torch.int32).cuda()
    tr = DetectorTrainer(det, lr=1e-3)
    mine = [tr.step(rt.Ragged(x, lengths), bits)[0] for _ in range(3)]
    lerr = float(np.abs(np.asarray(mine) - np.asarray(l64)).max())
    print(f"{name} {batch}: trainer losses {mine}, float64 {l64}: max err {lerr:.1e} (float32 restatement {lfloor:.1e}, "
          f"bound {bound(lfloor):.1e})")
    assert lerr <= bound(lfloor), (mine, l64)
    assert mine[2] < mine[0]
    tr.sync_host()
    for l, ref in enumerate(w64):
        err = H.rel(torch.from_numpy(net.weights[l]), ref)
        moved = float(np.abs(net.weights[l] - before[l]).max())
        print(f"{name} {batch} layer {l}: weights after 3 steps rel L2 {err:.2e} (float32 restatement {wfloors[l]:.1e}, "
              f"bound {bound(wfloors[l]):.1e}), moved by up to {moved:.1e}")
        assert err <= bound(wfloors[l]), (l, err)
        assert moved > 1e-4
    fresh = rt.DetectorWeights(plan, net.mel_basis, net.weights, net.biases)
    assert_same_detector(rt, plan, net.device_weights(plan), fresh, f"{name} trained")
