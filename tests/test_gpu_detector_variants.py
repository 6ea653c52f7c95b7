"""GPU tests of the detector's architecture variants (activation / norm_layer / final_activation of detection_net_cfg) on
the staged route: against the reference's own outputs (tests/golden/detector_variants.npz), against a float64 restatement
(test_detector_variants_host.VariantDetector) on uniform and ragged batches under every conv pipe, the embed loop against
the reference-shaped plug-in loop and the reference's 400-step trajectories, the card architecture through
aware_detector_create_ex, the stereo service round trip, and the training extension's refusal.

Run on the MI355X box:  python -m pytest tests/test_gpu_detector_variants.py -m gpu -x -q
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import make_clip
from test_detector_variants_host import (FIXTURE, VariantDetector, fixture_magnitudes, push_extremes_sum, split_key,
                                         variant_keys)

pytestmark = pytest.mark.gpu

KINK = 1e-5          # |u| below this at a ReLU / LeakyReLU argument: the gradient may differ by a kink's worth
STAGED = ["gelu_instance_tanh", "relu_none_sigmoid", "swish_batch_tanh", "leaky_relu_instance_sigmoid", "relu_instance_relu"]


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
def plan(rt):
    from aware_amd.utils.audio import default_plan
    return default_plan()


@pytest.fixture(scope="module")
def fx():
    return np.load(FIXTURE)


def make_net(key):
    from aware_amd.detection import AWAREDetectorNet
    act, norm, fin = split_key(key)
    return AWAREDetectorNet(activation=act, norm_layer=norm, final_activation=fin)


def loss_for(net):
    return "push_sigmoid" if net.final_activation == "sigmoid" else "push_extremes"


def band_mags(rng, frames):
    """Random band-limited magnitudes [513, T] per clip."""
    out = []
    for T in frames:
        m = np.zeros((513, T), np.float32)
        z = rng.standard_normal((225, T, 2))
        m[32:257] = 0.3 * np.hypot(z[..., 0], z[..., 1])
        out.append(m)
    return out


def check_gradient(mine, ref, kink, what, tight):
    """Relative L2 per clip; a clip with a ReLU / LeakyReLU argument within KINK of 0 gets the kink bound 2e-2."""
    rel = float(np.linalg.norm(mine - ref) / max(np.linalg.norm(ref), 1e-30))
    bound = tight if kink > KINK else 2e-2
    print(f"{what}: gradient rel L2 {rel:.2e} (kink {kink:.1e}, bound {bound:.0e})")
    assert rel < bound, (what, rel, kink)


@pytest.mark.parametrize("key", variant_keys())
def test_forward_and_gradient_vs_reference(rt, fx, key):
    """AWAREDetectorNet.forward and its magnitude gradient (plug-in seam: aware_detector_forward / _backward) against the
    reference's float32 CPU run of the same variant."""
    net = make_net(key)
    mag = torch.from_numpy(fixture_magnitudes()).cuda().requires_grad_(True)
    pred = net.forward(mag)
    np.testing.assert_allclose(pred.detach().cpu().numpy(), fx[f"net/{key}/pred"], atol=5e-5)
    push_extremes_sum(pred, torch.from_numpy(fx["target"]).cuda()).backward()
    g = mag.grad.cpu().numpy()[:, 32:257, ::int(fx["grad_step"])]             # the fixture keeps every 8th frame
    kink = VariantDetector(net).kink_distance(torch.from_numpy(fixture_magnitudes()).double())
    for b in range(g.shape[0]):
        check_gradient(g[b], fx[f"net/{key}/grad"][b], kink[b], f"{key} clip {b}", 2e-4)


@pytest.mark.parametrize("key", [k for k in variant_keys() if k != "leaky_relu_instance_tanh"])
@pytest.mark.parametrize("lengths", [[16000] * 32, [16000, 160000, 48000, 100001, 23456, 131072]])
def test_detector_entry_points_vs_float64(rt, plan, key, lengths):
    """aware_detector_forward / _backward of a variant on a 32-clip uniform batch and a ragged 1 - 10 s batch against the
    float64 restatement: values to 5e-5, the magnitude gradient of push_extremes per clip to 1e-4 relative L2."""
    net = make_net(key)
    dev = net.device_weights(plan)
    assert not dev.is_card
    batch = rt.Batch(lengths)
    rng = np.random.default_rng(len(lengths))
    mags = band_mags(rng, batch.frames)
    rows = torch.zeros((batch.total_frames, rt.SPEC_STRIDE), dtype=torch.float32)
    for i, m in enumerate(mags):
        rows[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :225] = torch.from_numpy(m[32:257].T)
    rows = rows.cuda()
    target = torch.from_numpy(np.where(rng.integers(0, 2, (batch.B, 20)) > 0, 1.0, -1.0).astype(np.float32))
    vals = rt.detector_forward(plan, dev, batch, rows)
    # dL/dpred of the per-clip push_extremes sum, from the device values
    p = vals.detach().clone().requires_grad_(True)
    push_extremes_sum(p, target.cuda()).backward()
    vals2, gmag = rt.detector_backward(plan, dev, batch, rows, p.grad)
    vals, vals2, gmag = vals.cpu().numpy(), vals2.cpu().numpy(), gmag.cpu().numpy()
    np.testing.assert_array_equal(vals, vals2)
    vd = VariantDetector(net)
    for i, m in enumerate(mags):
        x = torch.from_numpy(m).double()[None].requires_grad_(True)
        ref = vd.forward(x)
        push_extremes_sum(ref, target[i:i + 1].double()).backward()
        np.testing.assert_allclose(vals[i], ref.detach().numpy()[0], atol=5e-5)
        mine = gmag[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :225].T
        check_gradient(mine, x.grad.numpy()[0, 32:257], vd.kink_distance(x.detach())[0], f"{key} clip {i} (T {batch.frames[i]})",
                       1e-4)


def oracle_first_iteration(O, net, clip, wm_row, loss):
    """Loss, prediction, dL/dcoef [225, T] of the reference-shaped loop's first iteration (multibit_embedder.py:95-111) in
    float64 autograd, with the variant's network; and the clip's kink distance."""
    emb = O.Embedder(loss=loss, dtype=torch.float64)
    emb.det = VariantDetector(net, torch.float64)
    a = torch.from_numpy(clip).double()[None]
    mag0, phase = emb.analyse(a)
    c0 = mag0[:, emb.band].clone().requires_grad_(True)
    l, p = emb.forward_loss(c0, mag0, phase, torch.from_numpy(wm_row).double()[None])
    l.sum().backward()
    with torch.no_grad():
        mag = mag0.clone()
        mag2, _ = emb.recompute_magnitude(mag, phase)
        mag2[:, emb.nonband] = 0.0
    return float(l.detach()), p[0].detach().numpy(), c0.grad[0].numpy(), emb.det.kink_distance(mag2)[0]


@pytest.mark.parametrize("key", STAGED[:3])
@pytest.mark.parametrize("pipe", ["f16x2", "f32", "bf16x3"])
@pytest.mark.parametrize("lengths,sample", [([16000] * 32, [0, 13, 31]), ([16000, 160000, 48000, 100001, 23456], [0, 1, 2, 3, 4])])
def test_first_embed_gradient_vs_float64(rt, plan, O, key, pipe, lengths, sample):
    """aware_embed_gradient (the embed loop's first iteration) of a variant against float64 autograd of the reference-shaped
    loop, on every conv pipe: loss to 2e-5, prediction to 5e-5, dL/dcoef per clip to 1e-4 relative L2 (kink-checked)."""
    from aware_amd.detection import AWAREDetectorNet  # noqa: F401
    net = make_net(key)
    loss = loss_for(net)
    pairs = [make_clip(500 + i, n) for i, n in enumerate(lengths)]
    wm = np.stack([O.bits_to_bipolar(p[1]) for p in pairs]).astype(np.float32)
    batch = rt.Batch(lengths)
    sess = rt.EmbedSession(plan, net.device_weights(plan), batch, use_graph=False, conv_pipe=pipe, loss=loss)
    sess.begin(batch.pack([p[0] for p in pairs]), torch.from_numpy(wm).cuda())
    g = sess.gradient().cpu().numpy()
    lv, pv = sess.loss.cpu().numpy(), sess.pred.cpu().numpy()
    for i in sample:
        l, p, ref, kink = oracle_first_iteration(O, net, pairs[i][0], wm[i], loss)
        mine = g[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :225].T
        print(f"{key} {pipe} clip {i}: loss err {abs(lv[i] - l):.1e}, pred err {np.max(np.abs(pv[i] - p)):.1e}")
        assert abs(lv[i] - l) < 2e-5, (i, lv[i], l)
        np.testing.assert_allclose(pv[i], p, atol=5e-5)
        check_gradient(mine, ref, kink, f"{key} {pipe} clip {i}", 1e-4)


@pytest.mark.parametrize("key", ["gelu_instance_tanh", "relu_batch_sigmoid"])
def test_reference_shaped_loop_matches_fused_loop(rt, key):
    """Five iterations of AWAREEmbedder._optimize as the reference writes it (plug-in lists, the variant net under autograd,
    loss.backward(), NAdam + clamp) against the fused session on the same clip (tests/test_gpu_seam.py's bands)."""
    from aware_amd.embedding import AWAREEmbedder
    from aware_amd.embedding.losses import get_loss_fn
    from aware_amd.utils.audio import get_plan
    from oracle import aware_oracle as O
    act, norm, fin = split_key(key)
    loss_name = "push_sigmoid" if fin == "sigmoid" else "push_extremes"
    emb = AWAREEmbedder(detection_net_cfg=dict(activation=act, norm_layer=norm, final_activation=fin), loss=loss_name,
                        verbose=False)
    audio, bits = make_clip(1, 16000)
    target = torch.from_numpy(O.bits_to_bipolar(bits).astype(np.float32)).cuda()
    pre, post = emb.audio_preprocess_pipeline, emb.audio_postprocess_pipeline
    v = torch.from_numpy(audio).cuda()
    for p in pre:
        v = p(v)
    magnitude, phase = v
    fi, nfi = emb._get_embedding_frequency_indices(16000, 1024)
    fi_t, nfi_t = torch.from_numpy(fi).cuda(), torch.from_numpy(nfi).cuda()
    c0 = magnitude[fi_t].flatten().detach().clone()
    delta = c0 * 10 ** (-emb.tolerance_db / 20)
    lo, hi = torch.clamp(c0 - delta, min=0), c0 + delta
    coeffs = c0.clone().requires_grad_(True)
    opt = rt.NAdamClamp(coeffs.data, lr=0.1)
    loss_fn = get_loss_fn(loss_name)
    losses, grad1 = [], None
    for it in range(5):
        coeffs.grad = None
        wmag = magnitude.detach().clone()
        wmag[fi_t] = coeffs.reshape(len(fi), -1)
        d = (wmag, phase.detach())
        for p in post:
            d = p(*d) if isinstance(d, tuple) else p(d)
        for p in pre:
            d = p(*d) if isinstance(d, tuple) else p(d)
        m2 = d[0].clone()
        m2[nfi_t] = 0.0
        pred = emb.detection_net(m2.unsqueeze(0)).squeeze()
        loss = loss_fn(pred, target)
        loss.backward()
        if it == 0:
            grad1 = coeffs.grad.detach().clone()
        opt.step(coeffs.grad, lo, hi)
        losses.append(float(loss))
    get_plan()
    batch = rt.Batch([16000])
    sess = emb.start_session(batch, 16000)
    sess.begin(batch.pack([audio]), target[None])
    gf = sess.gradient()[:, :225].T.flatten()
    fused = []
    for it in range(5):
        sess.iterate(1)
        fused.append(float(sess.loss.cpu()[0]))
    assert abs(losses[0] - fused[0]) < 5e-6, (losses[0], fused[0])
    rel = float((grad1 - gf).norm() / gf.norm())
    print(key, "first gradient, plug-in seam vs fused loop, rel L2:", rel, "| losses", losses, fused)
    assert rel < 5e-5, rel
    assert np.max(np.abs(np.asarray(losses) - np.asarray(fused))) < 1e-3
    cf = sess.coef[:, :225].T.flatten()
    frac = float(((coeffs.detach() - cf).abs() <= 1e-3 * (1 + cf.abs())).float().mean())
    print(key, "coefficients equal after 5 steps:", frac)
    assert frac > 0.995
    lo_s, hi_s = sess.bounds
    c = sess.coef[:, :225]
    assert bool(((c >= lo_s[:, :225]) & (c <= hi_s[:, :225])).all())


@pytest.mark.parametrize("key", ["gelu_instance_tanh", "relu_batch_sigmoid"])
def test_embed_trajectory_400_steps_vs_reference(rt, plan, fx, key):
    """The reference's own 400-step embed of the 1 s seed clip with this variant (push_sigmoid for the sigmoid head): every
    step's loss within 1.6e-2, the watermarked waveform within 0.15 relative L2, the detected bits equal."""
    from oracle import aware_oracle as O
    net = make_net(key)
    audio, bits = make_clip(1, 16000)
    wm = O.bits_to_bipolar(bits).astype(np.float32)[None]
    batch = rt.Batch([16000])
    sess = rt.EmbedSession(plan, net.device_weights(plan), batch, use_graph=True, loss=loss_for(net))
    sess.begin(batch.pack([audio]), torch.from_numpy(wm).cuda())
    mine = []
    for _ in range(400):
        sess.iterate(1)
        mine.append(float(sess.loss.cpu()[0]))
    ref = fx[f"traj/{key}/losses"]
    d = np.abs(np.asarray(mine) - ref)
    print(f"{key}: |loss - reference| step0 {d[0]:.2e} first20 {d[:20].max():.2e} max {d.max():.2e} (step {d.argmax()})")
    assert d[0] < 1e-5
    assert d.max() <= 1.6e-2
    out = sess.finish(torch.tensor([float(np.max(audio))], device="cuda"))
    out_c = out.cpu().numpy()
    assert out_c.shape[0] == int(fx[f"traj/{key}/out_len"])
    r = fx[f"traj/{key}/out_sample"]
    rel = np.linalg.norm(out_c[::int(fx[f"traj/{key}/out_step"])] - r) / np.linalg.norm(r)
    print(f"{key}: relative L2 distance to the reference's watermarked audio {rel:.3e}")
    assert rel <= 0.15
    vals = rt.detect(plan, net.device_weights(plan), rt.Batch([out_c.shape[0]]), out).cpu().numpy()[0]
    print(f"{key}: max |raw - reference raw_marked| {np.max(np.abs(vals - fx[f'traj/{key}/raw_marked'])):.2e}")
    np.testing.assert_array_equal(O.decode_bits(vals), fx[f"traj/{key}/det_bits"])


def test_create_ex_with_the_card_architecture_is_create(rt, plan, O):
    """aware_detector_create_ex with {leaky_relu, instance, tanh} builds the model card's detector: detection and the embed
    loop's first gradient and 3 iterations bit-identical to aware_detector_create's."""
    from aware_amd.detection import AWAREDetectorNet
    net = AWAREDetectorNet()
    ex = rt.DetectorWeights(plan, net.mel_basis, net.weights, net.biases, arch=net.architecture())
    old = rt.DetectorWeights(plan, net.mel_basis, net.weights, net.biases)
    assert ex.is_card and old.is_card
    lengths = [48000, 16000, 30000, 160000]
    pairs = [make_clip(40 + i, n) for i, n in enumerate(lengths)]
    batch = rt.Batch(lengths)
    audio = batch.pack([p[0] for p in pairs])
    np.testing.assert_array_equal(rt.detect(plan, ex, batch, audio).cpu().numpy(), rt.detect(plan, old, batch, audio).cpu().numpy())
    wm = torch.from_numpy(np.stack([O.bits_to_bipolar(p[1]) for p in pairs]).astype(np.float32)).cuda()
    res = []
    for d in (ex, old):
        sess = rt.EmbedSession(plan, d, batch, use_graph=True)
        sess.begin(audio, wm)
        g = sess.gradient().cpu().numpy()
        sess.iterate(3)
        res.append((g, sess.coef.cpu().numpy(), sess.loss.cpu().numpy()))
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


def test_stereo_service_round_trip(rt):
    """embed_watermark / detect_watermark of a stereo clip through load()-style objects with a variant network: finite
    outputs of the right shape, every coefficient of the loop inside its box."""
    from aware_amd.detection import AWAREDetector
    from aware_amd.embedding import AWAREEmbedder
    from aware_amd.service import detect_watermark, embed_watermark
    cfg = dict(activation="swish", norm_layer="batch", final_activation="tanh")
    emb = AWAREEmbedder(detection_net_cfg=cfg, loss="push_extremes", num_iterations=40, verbose=False)
    det = AWAREDetector(model=emb.detection_net)
    left, bits = make_clip(7, 24000)
    right, _ = make_clip(8, 24000)
    out = embed_watermark(np.column_stack([left, right]), 16000, bits, emb)
    assert out.shape == (256 * (1 + 24000 // 256 - 1), 2) and np.isfinite(out).all()
    got = detect_watermark(out, 16000, det)
    assert np.asarray(got).shape == (20,)
    batch = rt.Batch([24000, 24000])
    from aware_amd.utils.audio import default_plan
    sess = rt.EmbedSession(default_plan(), emb.detection_net.device_weights(default_plan()), batch, num_iterations=40)
    sess.begin(batch.pack([left, right]), torch.ones((2, 20), device="cuda"))
    sess.iterate(40)
    lo, hi = sess.bounds
    c = sess.coef[:, :225]
    assert bool(torch.isfinite(sess.loss).all())
    assert bool(((c >= lo[:, :225]) & (c <= hi[:, :225])).all())


def test_training_extension_refuses_a_variant(rt, plan):
    """DetectorTrainer and aware_detector_*_gradients / _update* serve the model card's network only."""
    net = make_net("gelu_instance_tanh")
    dev = net.device_weights(plan)
    batch = rt.Batch([16000])
    mag = torch.zeros((batch.total_frames, rt.SPEC_STRIDE), device="cuda")
    with pytest.raises(NotImplementedError):
        rt.detector_train_gradients(plan, dev, batch, mag, torch.ones((1, 20), device="cuda"))
    with pytest.raises(NotImplementedError):
        rt.detector_weight_gradients(plan, dev, batch, mag, torch.ones((1, 20), device="cuda"))
    with pytest.raises(NotImplementedError):
        dev.update(net.weights, net.biases)
    # the C ABI itself: AWARE_E_UNSUPPORTED before any work (every pointer argument non-null)
    lib = dev.lib
    t = torch.zeros(16, device="cuda")
    ptrs = (C.c_void_p * 4)(*([t.data_ptr()] * 4))
    p = C.c_void_p(t.data_ptr())
    assert lib.aware_detector_train_gradients(dev.h, batch.h, p, p, 0, p, p, p, ptrs, ptrs, p, 64, None) == -2
    assert lib.aware_detector_weight_gradients(dev.h, batch.h, p, p, p, p, ptrs, ptrs, p, 64, None) == -2
    assert lib.aware_detector_update_device(dev.h, ptrs, ptrs, None) == -2
