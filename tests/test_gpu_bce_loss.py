"""GPU tests of the loss bce (AWARE_LOSS_BCE, csrc/common.hpp::loss_term_bce) on detectors that end in sigmoid: the first
loop body against float64 torch on the narrow and the wide read-out and both conv pipes, saturated predictions, the routes a
sigmoid detector can take (temporal convolutions, another initial pool, the general geometry), the refusals, the unipolar
configuration end to end (embed_batch, detect_batch, PatternDecoder, the service), and a loop chain.

The restatements (SigmoidDetector, UnipolarLoop, first_iteration) and the CPU run's figures are tests/test_bce_loss_host.py's.
Bounds of the first step: those tests/test_gpu_detector_variants.py applies to push_sigmoid on a sigmoid net -- loss 2e-5,
prediction 5e-5, dL/dcoef 1e-4 relative L2 per clip (gelu blocks: no kink); on the general route the bounds
tests/test_gpu_general_geometry.py applies there (loss 5e-5 max(1, |loss|), gradient 2e-3 on the default pipe).

Run on the MI355X box:  python -m pytest tests/test_gpu_bce_loss.py -m gpu -x -q -s
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import make_clip
from test_bce_loss_host import (CPU_RUN, E2E_NET, NET, PAYLOAD, SPREAD_DEV, STEPS, SigmoidDetector, UnipolarLoop,
                                first_iteration, make_net, payload_bits)

pytestmark = pytest.mark.gpu

LOSSES = ("bce", "push_sigmoid")
RAGGED = [16000, 513, 12345]         # 1 s; one pooled frame (three frames); odd T
ROUTE_CLIPS = [8192, 5000]


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


def targets(seed, B, n_bits):
    return np.random.default_rng(seed).integers(0, 2, (B, n_bits)).astype(np.float32)


def device_first_step(rt, plan, net, batch, clips, wm, loss, pipe="f16x2"):
    """(per-clip loss, prediction, gradient rows) of aware_embed_gradient after begin()."""
    sess = rt.EmbedSession(plan, net.device_weights(plan), batch, use_graph=False, conv_pipe=pipe, loss=loss)
    sess.begin(batch.pack(clips), torch.from_numpy(wm).cuda())
    g = sess.gradient()
    torch.cuda.synchronize()
    return sess.loss.cpu().numpy().copy(), sess.pred.cpu().numpy().copy(), g.cpu().numpy()


_REF = {}


def reference(key, net, clips, wm, bands=(500, 4000)):
    """float64 autograd of the loop's first body per clip and loss: computed once per case, shared by the pipes.  A clip whose
    synthesis torch.stft cannot pad (513 samples: 512 out) has no loop in torch; its entry is None."""
    if key not in _REF:
        out = {}
        for loss in LOSSES:
            loop = UnipolarLoop(net, loss, torch.float64, bands)
            out[loss] = [first_iteration(loop, c, wm[i]) if loop.hop * (len(c) // loop.hop) > loop.n_fft // 2 else None
                         for i, c in enumerate(clips)]
        _REF[key] = out
    return _REF[key]


def one_pooled_frame(net, loss, target):
    """What the restatement reads for a clip of one pooled frame, whatever its magnitudes: every block's InstanceNorm over
    one frame is 0, so the prediction is sigmoid(0) and no gradient reaches the magnitudes.  (loss, prediction, max |grad|)."""
    mag = torch.rand((1, net.n_fft // 2 + 1, 3), dtype=torch.float64).requires_grad_(True)
    p = SigmoidDetector(net).forward(mag)
    loop = UnipolarLoop(net, loss, torch.float64)
    l = loop.loss(p, torch.from_numpy(target).double()[None])
    l.sum().backward()
    return float(l.detach()), p[0].detach().numpy(), float(mag.grad.abs().max())


def compare(what, batch, nband, mine, ref, bounds, zero=None, relative_loss=False):
    """Print every figure, then assert.  mine: (loss, pred, grad rows); ref: per clip (loss, pred, grad [nband, T]) or None
    with zero[i] = (loss, pred) of a clip whose gradient is exactly 0.  relative_loss: the loss error over max(1, |loss|)."""
    lv, pv, g = mine
    bl, bp, bg = bounds
    figures = []
    for i, r in enumerate(ref):
        rows = g[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :nband].T
        if r is None:
            l, p = zero[i]
            figures.append((i, abs(float(lv[i]) - l), float(np.max(np.abs(pv[i] - p))), float(np.abs(rows).max()), True))
        else:
            l, p, gr = r
            figures.append((i, abs(float(lv[i]) - l) / (max(1.0, abs(l)) if relative_loss else 1.0), float(np.max(np.abs(pv[i] - p))),
                            float(np.linalg.norm(rows - gr) / np.linalg.norm(gr)), False))
        i, el, ep, eg, z = figures[-1]
        print(f"{what} clip {i}: loss err {el:.1e} (bound {bl:.0e}), pred err {ep:.1e} (bound {bp:.0e}), gradient "
              f"{'max |g| %.1e (must be 0)' % eg if z else 'rel L2 %.2e (bound %.0e)' % (eg, bg)}")
    assert np.isfinite(g).all() and (g.shape[1] == nband or float(np.abs(g[:, nband:]).max()) == 0.0)
    for i, el, ep, eg, z in figures:
        assert el < bl and ep < bp, (what, i, el, ep)
        assert eg == 0.0 if z else eg < bg, (what, i, eg)


# ---- 1. the first step -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("n_bits", [20, 40])
def test_first_step_vs_float64(rt, plan, n_bits, pipe):
    """Per-clip loss, prediction and aware_embed_gradient of bce on the ragged batch against float64 autograd, on the narrow
    read-out (20 bits, head_kernel) and the wide one (40 bits, readout_wide_kernel), by push_sigmoid's bounds; push_sigmoid on
    the same inputs is printed and held to them too.  The 513-sample clip reads what the restatement reads for one pooled
    frame: prediction 0.5, loss ln 2, gradient exactly 0."""
    net = make_net(**NET, output_length=n_bits)
    clips = [make_clip(900 + i, n)[0] for i, n in enumerate(RAGGED)]
    wm = targets(n_bits, len(RAGGED), n_bits)
    batch = rt.Batch(RAGGED)
    ref = reference(("card", n_bits), net, clips, wm)
    for loss in LOSSES:
        l1, p1, g1 = one_pooled_frame(net, loss, wm[1])
        assert g1 == 0.0 and np.all(p1 == 0.5)
        if loss == "bce":
            assert abs(l1 - np.log(2.0)) < 1e-12
        mine = device_first_step(rt, plan, net, batch, clips, wm, loss, pipe)
        compare(f"{loss} {n_bits} bits {pipe}", batch, 225, mine, ref[loss], (2e-5, 5e-5, 1e-4), zero={1: (l1, p1)})


# ---- 2. saturation -----------------------------------------------------------------------------------------------------
def saturated_net(n_bits, clips):
    """The first-step net without the block norm (behind InstanceNorm a scaled weight changes nothing), its last block's
    weights scaled until the float32 restatement reads every bit of every clip as exactly 0 or 1 with |logit| > 150 (the
    device's logits differ in the last digits, and sigmoid is exactly 0 only below -88.8); and those predictions."""
    net = make_net(**dict(NET, norm_layer="none"), output_length=n_bits)
    base = net.weights[-1].copy()
    scale = 1.0
    for _ in range(40):
        net.weights[-1] = (base * np.float32(scale)).astype(np.float32)
        loop = UnipolarLoop(net, "bce")
        ps, xs = [], []
        with torch.no_grad():
            for c in clips:
                mag0, phase = loop.analyse(torch.from_numpy(c)[None])
                mag2, _ = loop.recompute_magnitude(mag0, phase)
                mag2[:, loop.nonband] = 0.0
                xs.append(loop.det.logits(mag2)[0].numpy())
                ps.append(loop.det.forward(mag2)[0].numpy())
        if min(float(np.abs(x).min()) for x in xs) > 150.0:
            return net, np.stack(ps), scale
        scale *= 4.0
    raise AssertionError("no scale saturates every bit")


@pytest.mark.parametrize("n_bits", [20, 40])
def test_saturated_predictions(rt, plan, n_bits):
    """Every prediction exactly 0 or 1 and the targets wrong on every other bit: the loss is the clamp's 100 per wrong bit
    (50 per clip, to float32 summation), every gradient value is finite, and the gradient is exactly 0, as the restatement's
    (sigmoid' = p (1 - p) = 0 times the finite 1e12 / n_bits)."""
    lengths = [16000, 12345]
    clips = [make_clip(900 + i, n)[0] for i, n in enumerate(lengths)]
    net, p_sat, scale = saturated_net(n_bits, clips)
    assert np.all((p_sat == 0.0) | (p_sat == 1.0)) and 0.0 < p_sat.mean() < 1.0
    wm = p_sat.copy()
    wm[:, 1::2] = 1.0 - wm[:, 1::2]
    loop = UnipolarLoop(net, "bce")
    batch = rt.Batch(lengths)
    for i, c in enumerate(clips):
        l, p, g = first_iteration(loop, c, wm[i])
        assert np.array_equal(p, p_sat[i]) and abs(l - 50.0) < 1e-4 and np.isfinite(g).all() and float(np.abs(g).max()) == 0.0
    for pipe in ("f16x2", "bf16x3"):
        lv, pv, g = device_first_step(rt, plan, net, batch, clips, wm, "bce", pipe)
        print(f"saturated, {n_bits} bits, scale {scale:g}, {pipe}: losses {lv.tolist()}, max |g| {np.abs(g).max():.1e}")
        assert np.array_equal(pv, p_sat)
        assert np.all(np.abs(lv - 50.0) < 50.0 * n_bits * 2.0 ** -23), lv
        assert np.isfinite(g).all() and float(np.abs(g).max()) == 0.0


# ---- 3. the routes -----------------------------------------------------------------------------------------------------
ROUTES = {
    "taps": dict(net=dict(NET, output_length=20, temporal_convs=True, kernel_size=3, padding=1), emb={}),
    "pool": dict(net=dict(NET, output_length=40, initial_pools=True, initial_pool_size=3, initial_pool_stride=2), emb={}),
    "general": dict(net=dict(NET, output_length=20, n_fft=512),
                    emb=dict(general_geometry=True, frame_length=512, hop_length=128, win_length=512)),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_routes_first_step(rt, route):
    """One first step each: temporal convolutions with 20 bits (the TapRows read-out), a (3, 2) initial pool with 40 bits (the
    wide read-out with POOL), and the general route at 512 / 128 / 512, through AWAREEmbedder's own session."""
    from aware_amd.embedding import AWAREEmbedder
    cfg = ROUTES[route]
    emb = AWAREEmbedder(pattern_mode="bytes2bits", loss="bce", verbose=False, use_graph=False, detection_net_cfg=dict(cfg["net"]),
                        **cfg["emb"])
    net = emb.detection_net
    n_bits = net.output_length
    clips = [make_clip(950 + i, n)[0] for i, n in enumerate(ROUTE_CLIPS)]
    wm = targets(7, len(clips), n_bits)
    batch = emb.make_batch(ROUTE_CLIPS, 16000)
    eplan = emb._plan(16000)
    assert eplan.general == (route == "general") and not net.is_card_arch
    sess = emb.start_session(batch, 16000)
    sess.begin(batch.pack(clips), torch.from_numpy(wm).cuda())
    g = sess.gradient()
    torch.cuda.synchronize()
    mine = (sess.loss.cpu().numpy().copy(), sess.pred.cpu().numpy().copy(), g.cpu().numpy())
    ref = reference(route, net, clips, wm)["bce"]
    bounds = (5e-5, 5e-5, 2e-3) if route == "general" else (2e-5, 5e-5, 1e-4)
    compare(f"bce {route}", batch, eplan.nband if route == "general" else 225, mine, ref, bounds, relative_loss=route == "general")


# ---- 4. refusals -------------------------------------------------------------------------------------------------------
def test_refusals(rt, plan):
    from aware_amd._lib import EmbedConfig
    from aware_amd.detection import AWAREDetector, AWAREDetectorNet
    from aware_amd.embedding import AWAREEmbedder
    from aware_amd.training import DetectorTrainer
    lib = plan.lib
    batch = rt.Batch([16000])
    h = C.c_void_p()

    def create(dev, loss):
        n = lib.aware_embed_workspace_bytes(batch.h, dev.h)
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        cfg = EmbedConfig(5, 6.0, loss, 0.1, 0.9, 0.999, 1e-8, 4e-3, 0, 0, 0, 0, 0.0, 0, 0)
        rc = lib.aware_embed_create(C.byref(h), plan.h, dev.h, batch.h, C.byref(cfg), rt._ptr(ws), n, rt._stream())
        if rc == 0:
            lib.aware_embed_destroy(h)
        return rc

    card = AWAREDetectorNet()
    for net in (card, make_net(**dict(NET, final_activation="tanh")), make_net(**dict(NET, final_activation="relu"))):
        assert create(net.device_weights(plan), 8) == -2                   # AWARE_E_UNSUPPORTED
    sig = make_net(**NET).device_weights(plan)
    assert create(sig, 8) == 0
    assert create(sig, 7) == -1 and create(sig, 9) == -1                  # the external kind is internal; nothing behind 8
    with pytest.raises(rt.AwareHipError, match="unsupported"):
        rt.EmbedSession(plan, card.device_weights(plan), batch, loss="bce")
    emb = AWAREEmbedder(pattern_mode="bytes2bits", loss="bce", verbose=False, detection_net_cfg=dict(E2E_NET))
    wm = payload_bits().astype(np.float32)
    wm[3] = 2.0
    with pytest.raises(ValueError, match="between 0 and 1"):
        emb.embed_batch([make_clip(0, 16000)[0]], 16000, wm[None])
    # training: the sigmoid detector is not the card's, and the card's detector does not take bce
    with pytest.raises(NotImplementedError):
        DetectorTrainer(AWAREDetector(emb.detection_net, threshold=0.5, pattern_mode="bytes2bits"))
    mag = torch.zeros((batch.total_frames, rt.SPEC_STRIDE), device="cuda")
    tg = torch.zeros((1, 20), device="cuda")
    with pytest.raises(NotImplementedError, match="bce"):
        rt.detector_train_gradients(plan, card.device_weights(plan), batch, mag, tg, "bce")
    n = lib.aware_detector_train_workspace_bytes(batch.h, card.device_weights(plan).h)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    vals, losses = torch.empty((1, 20), device="cuda"), torch.empty((1,), device="cuda")
    ch = card.channels
    gw = [torch.empty((ch[i + 1], ch[i]), device="cuda") for i in range(len(ch) - 1)]
    gb = [torch.empty((ch[i + 1],), device="cuda") for i in range(len(ch) - 1)]
    pw = (C.c_void_p * len(gw))(*[t.data_ptr() for t in gw])
    pb = (C.c_void_p * len(gb))(*[t.data_ptr() for t in gb])
    assert lib.aware_detector_train_gradients(card.device_weights(plan).h, batch.h, rt._ptr(mag), rt._ptr(tg), 8, rt._ptr(losses),
                                              rt._ptr(vals), None, pw, pb, rt._ptr(ws), n, rt._stream()) == -1


# ---- 5. end to end -----------------------------------------------------------------------------------------------------
def test_end_to_end_unipolar(rt):
    """The unipolar configuration on the CPU run's four clips: embed_batch (400 steps) -> detect_batch -> PatternDecoder at
    threshold 0.5, with bce and with push_sigmoid.  The device's mean |v - 0.5| lies as near the CPU run's as push_sigmoid's
    own device run lies to its CPU twin (measured here, on the same clips) plus the two spreads the CPU test allows a clip;
    the wrong bits are no more than the CPU run's plus that device-to-CPU difference of push_sigmoid, and per clip no more
    than push_sigmoid's on the device plus one.  Then one mono clip through service.embed_watermark / detect_watermark, and
    WatermarkPipeline, which reads the bits at detector.threshold."""
    from aware_amd.detection import AWAREDetector
    from aware_amd.embedding import AWAREEmbedder
    from aware_amd.pipeline import WatermarkPipeline
    from aware_amd.service import detect_watermark, embed_watermark
    from aware_amd.utils.watermark import PatternDecoder, PatternEncoder
    clips = [make_clip(s, 16000)[0] for s in range(4)]
    bits = payload_bits()
    wm = np.tile(PatternEncoder(mode="bytes2bits")(PAYLOAD).astype(np.float32), (4, 1))
    decode = PatternDecoder(threshold=0.5, encoder_mode="bytes2bits")
    got = {}
    for loss in LOSSES:
        emb = AWAREEmbedder(pattern_mode="bytes2bits", loss=loss, verbose=False, num_iterations=STEPS, detection_net_cfg=dict(E2E_NET))
        det = AWAREDetector(emb.detection_net, threshold=0.5, pattern_mode="bytes2bits")
        outs = emb.embed_batch(clips, 16000, wm)
        vals = det.detect_batch([o.cpu().numpy() for o in outs], 16000).cpu().numpy()
        wrong = np.array([(np.frombuffer(decode(v), dtype=np.uint8) != bits).sum() for v in vals])
        got[loss] = (wrong, float(np.abs(vals - 0.5).mean()), emb, det)
        print(f"{loss}: wrong bits per clip {wrong.tolist()} (CPU {CPU_RUN[loss][0]}), mean |v - 0.5| {got[loss][1]:.4f} "
              f"(CPU {CPU_RUN[loss][1]:.4f})")
    twin_dev = abs(got["push_sigmoid"][1] - CPU_RUN["push_sigmoid"][1])
    twin_bits = abs(int(got["push_sigmoid"][0].sum()) - 4 * CPU_RUN["push_sigmoid"][0])
    print(f"push_sigmoid device against its CPU twin: mean |v - 0.5| {twin_dev:.4f}, wrong bits {twin_bits}")
    wrong, dev, emb, det = got["bce"]
    assert abs(dev - CPU_RUN["bce"][1]) <= twin_dev + 2 * SPREAD_DEV, (dev, twin_dev)
    assert int(wrong.sum()) <= 4 * CPU_RUN["bce"][0] + twin_bits, wrong
    assert np.all(wrong <= got["push_sigmoid"][0] + 1), (wrong, got["push_sigmoid"][0])
    # the service on one mono clip
    marked = embed_watermark(clips[0], 16000, PAYLOAD, emb)
    assert marked.shape == (15872,) and np.isfinite(marked).all()
    read = detect_watermark(marked, 16000, det)
    service_wrong = int((np.frombuffer(read, dtype=np.uint8) != bits).sum())
    print(f"service: wrong bits {service_wrong}")
    assert service_wrong <= int(wrong[0]) + 1
    # the pipeline takes the bits themselves as targets and reports the errors at detector.threshold
    emb.num_iterations = STEPS
    res = WatermarkPipeline(emb, det).run(rt.Ragged.from_list(clips), torch.from_numpy(np.tile(bits, (4, 1))).cuda())
    want = torch.from_numpy(np.tile(bits, (4, 1))).cuda()
    assert torch.equal(res.bits, (res.values > 0.5).to(torch.int32))
    assert int(res.clean_bit_errors) == int((res.bits != want).sum())
    print(f"pipeline: wrong bits {int(res.clean_bit_errors)}")
    assert int(res.clean_bit_errors) <= int(wrong.sum()) + 4          # the same embed behind the service's rescale: a bit per clip


# ---- 6. with a loop chain ----------------------------------------------------------------------------------------------
def test_with_a_loop_chain(rt):
    """bce behind a loop chain (gaussian noise at 10 dB), five steps: finite losses, the fifth below the first, and the same
    five losses from a second session with the same seeds."""
    from aware_amd.embedding import AWAREEmbedder
    clips = [make_clip(s, 16000)[0] for s in range(2)]
    wm = np.tile(payload_bits().astype(np.float32), (2, 1))
    runs = []
    for _ in range(2):
        emb = AWAREEmbedder(pattern_mode="bytes2bits", loss="bce", verbose=False, num_iterations=5, loop_attack_seed=11,
                            loop_attacks=[{"kind": "gaussian_noise", "snr_db": 10}], detection_net_cfg=dict(E2E_NET))
        batch = emb.make_batch([16000, 16000], 16000)
        sess = emb.start_session(batch, 16000)
        sess.begin(batch.pack(clips), torch.from_numpy(wm).cuda())
        losses = []
        for _ in range(5):
            sess.iterate(1)
            losses.append(sess.loss.cpu().numpy().copy())
        runs.append(np.stack(losses))
    print(f"losses per step: {runs[0].tolist()}")
    assert np.isfinite(runs[0]).all() and np.all(runs[0][4] < runs[0][0])
    assert np.array_equal(runs[0], runs[1])
