"""GPU tests of payload lengths other than the model card's 20 bits (watermark_length / detection_net_cfg.output_length
1..512): the detector entry points, the embed loop's first gradient on both conv pipes, the reference's own 400-step embed at
64 bits, a variant architecture on the staged route, graph replay, silent clips, the training extension and the service.
Without the feature every one of them fails at aware_detector_create (AWARE_E_UNSUPPORTED) or at AWAREDetectorNet."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, make_clip
from test_detector_variants_host import VariantDetector, fixture_magnitudes, push_extremes_sum
from test_payload_length_host import LENGTHS, PayloadDetector

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "payload_lengths.npz")
KINK = 1e-5
RAGGED = [16000, 160000, 48000, 100001, 23456, 131072]


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


def make_net(L, **kw):
    from aware_amd.detection import AWAREDetectorNet
    return AWAREDetectorNet(output_length=L, **kw)


def band_mags(rng, frames):
    out = []
    for T in frames:
        m = np.zeros((513, T), np.float32)
        z = rng.standard_normal((225, T, 2))
        m[32:257] = 0.3 * np.hypot(z[..., 0], z[..., 1])
        out.append(m)
    return out


def check_gradient(mine, ref, kink, what, tight):
    """Relative L2 per clip; a clip with a LeakyReLU argument within KINK of 0 gets the kink bound 2e-2."""
    rel = float(np.linalg.norm(mine - ref) / max(np.linalg.norm(ref), 1e-30))
    bound = tight if kink > KINK else 2e-2
    print(f"{what}: gradient rel L2 {rel:.2e} (kink {kink:.1e}, bound {bound:.0e})")
    assert rel < bound, (what, rel, kink)


@pytest.mark.parametrize("L", LENGTHS)
def test_forward_and_gradient_vs_reference(rt, fx, L):
    """AWAREDetectorNet.forward and its magnitude gradient (plug-in seam) against the reference's float32 CPU run."""
    net = make_net(L)
    mag = torch.from_numpy(fixture_magnitudes()).cuda().requires_grad_(True)
    pred = net.forward(mag)
    assert tuple(pred.shape) == (2, L, 1)
    np.testing.assert_allclose(pred.detach().cpu().numpy(), fx[f"net/L{L}/pred"], atol=5e-5)
    push_extremes_sum(pred, torch.from_numpy(fx[f"net/L{L}/target"]).cuda()).backward()
    g = mag.grad.cpu().numpy()[:, 32:257, ::int(fx["grad_step"])]
    kink = VariantDetector(net).kink_distance(torch.from_numpy(fixture_magnitudes()).double())
    for b in range(g.shape[0]):
        check_gradient(g[b], fx[f"net/L{L}/grad"][b], kink[b], f"L {L} clip {b}", 2e-4)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("lengths,sample", [([16000] * 32, [0, 13, 31]), ([16000] * 256, [0, 100, 255]),
                                            (RAGGED, list(range(len(RAGGED))))])
def test_detector_entry_points_vs_float64(rt, plan, L, lengths, sample):
    """aware_detector_forward / _backward against the float64 restatement: uniform batches of 32 and 256 clips (the f16
    two-term conv kernels and, above 32 bits, the wide read-out) and a ragged 1 - 10 s batch: values to 5e-5, the
    magnitude gradient of push_extremes per clip to 1e-4 relative L2."""
    net = make_net(L)
    dev = net.device_weights(plan)
    assert dev.is_card and dev.n_bits == L
    batch = rt.Batch(lengths)
    rng = np.random.default_rng(len(lengths) + L)
    mags = band_mags(rng, batch.frames)
    rows = torch.zeros((batch.total_frames, rt.SPEC_STRIDE), dtype=torch.float32)
    for i, m in enumerate(mags):
        rows[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :225] = torch.from_numpy(m[32:257].T)
    rows = rows.cuda()
    target = torch.from_numpy(np.where(rng.integers(0, 2, (batch.B, L)) > 0, 1.0, -1.0).astype(np.float32))
    vals = rt.detector_forward(plan, dev, batch, rows)
    assert tuple(vals.shape) == (batch.B, L)
    p = vals.detach().clone().requires_grad_(True)
    push_extremes_sum(p, target.cuda()).backward()
    vals2, gmag = rt.detector_backward(plan, dev, batch, rows, p.grad)
    vals, vals2, gmag = vals.cpu().numpy(), vals2.cpu().numpy(), gmag.cpu().numpy()
    np.testing.assert_array_equal(vals, vals2)
    assert np.isfinite(gmag).all()
    ref_det = PayloadDetector(L)
    vd = VariantDetector(net)
    for i in sample:
        x = torch.from_numpy(mags[i]).double()[None].requires_grad_(True)
        ref = ref_det.forward(x)
        push_extremes_sum(ref, target[i:i + 1].double()).backward()
        np.testing.assert_allclose(vals[i], ref.detach().numpy()[0], atol=5e-5)
        mine = gmag[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :225].T
        check_gradient(mine, x.grad.numpy()[0, 32:257], vd.kink_distance(x.detach())[0], f"L {L} clip {i} (T {batch.frames[i]})",
                       1e-4)


def oracle_first_iteration(O, det64, kinker, clip, wm_row, loss):
    """Loss, prediction, dL/dcoef [225, T] of the reference-shaped loop's first iteration in float64 autograd with the L-bit
    detector; and the clip's kink distance."""
    emb = O.Embedder(loss=loss, dtype=torch.float64)
    emb.det = det64
    a = torch.from_numpy(clip).double()[None]
    mag0, phase = emb.analyse(a)
    c0 = mag0[:, emb.band].clone().requires_grad_(True)
    lv, p = emb.forward_loss(c0, mag0, phase, torch.from_numpy(wm_row).double()[None])
    lv.sum().backward()
    with torch.no_grad():
        mag2, _ = emb.recompute_magnitude(mag0.clone(), phase)
        mag2[:, emb.nonband] = 0.0
    return float(lv.detach()), p[0].detach().numpy(), c0.grad[0].numpy(), kinker.kink_distance(mag2)[0]


def payload(seed, B, L):
    return np.where(np.random.default_rng(seed).integers(0, 2, (B, L)) > 0, 1.0, -1.0).astype(np.float32)


@pytest.mark.parametrize("L", [21, 64, 128])
@pytest.mark.parametrize("pipe", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("lengths,sample", [([16000] * 32, [0, 31]), ([16000, 160000, 48000, 23456], [0, 1, 2, 3])])
def test_first_embed_gradient_vs_float64(rt, plan, O, L, pipe, lengths, sample):
    """aware_embed_gradient against float64 autograd of the reference-shaped loop with the L-bit detector: loss to 2e-5,
    prediction to 5e-5, dL/dcoef per clip to 1e-4 relative L2 (kink-checked)."""
    net = make_net(L)
    clips = [make_clip(700 + i, n)[0] for i, n in enumerate(lengths)]
    wm = payload(L, len(lengths), L)
    batch = rt.Batch(lengths)
    sess = rt.EmbedSession(plan, net.device_weights(plan), batch, use_graph=False, conv_pipe=pipe)
    sess.begin(batch.pack(clips), torch.from_numpy(wm).cuda())
    g = sess.gradient().cpu().numpy()
    lv, pv = sess.loss.cpu().numpy(), sess.pred.cpu().numpy()
    assert pv.shape == (len(lengths), L)
    det64, kinker = PayloadDetector(L), VariantDetector(net)
    for i in sample:
        l_ref, p_ref, ref, kink = oracle_first_iteration(O, det64, kinker, clips[i], wm[i], "push_extremes")
        mine = g[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :225].T
        print(f"L {L} {pipe} clip {i}: loss err {abs(lv[i] - l_ref):.1e}, pred err {np.max(np.abs(pv[i] - p_ref)):.1e}")
        assert abs(lv[i] - l_ref) < 2e-5, (i, lv[i], l_ref)
        np.testing.assert_allclose(pv[i], p_ref, atol=5e-5)
        check_gradient(mine, ref, kink, f"L {L} {pipe} clip {i}", 1e-4)


def test_push_extremes_l1_first_gradient_at_64_bits(rt, plan, O):
    """The push_extremes_l1 loss (per-clip L1 term added inside the read-out) at 64 bits: first loss against float64."""
    L, lam = 64, 0.5
    net = make_net(L)
    lengths = [16000] * 32
    clips = [make_clip(800 + i, n)[0] for i, n in enumerate(lengths)]
    wm = payload(5, len(lengths), L)
    batch = rt.Batch(lengths)
    sess = rt.EmbedSession(plan, net.device_weights(plan), batch, use_graph=False, loss="push_extremes_l1", l1_weight=lam)
    sess.begin(batch.pack(clips), torch.from_numpy(wm).cuda())
    g = sess.gradient().cpu().numpy()
    lv = sess.loss.cpu().numpy()
    emb = O.Embedder(loss="push_extremes_l1", dtype=torch.float64, l1_weight=lam)
    emb.det = PayloadDetector(L)
    for i in (0, 31):
        a = torch.from_numpy(clips[i]).double()[None]
        mag0, phase = emb.analyse(a)
        c0 = mag0[:, emb.band].clone().requires_grad_(True)
        l_ref, _ = emb.forward_loss(c0, mag0, phase, torch.from_numpy(wm[i]).double()[None])
        l_ref = float(l_ref.detach())
        assert abs(lv[i] - l_ref) < 2e-5, (i, lv[i], l_ref)
    assert np.isfinite(g).all()


def test_embed_trajectory_400_steps_vs_reference(rt, plan, fx, O):
    """The reference's own 400-step embed of the 1 s seed clip with a 64-bit payload: every step's loss within 1.6e-2, the
    watermarked waveform within 0.15 relative L2, the detected bits equal the reference's (and the payload)."""
    L = 64
    net = make_net(L)
    audio, _ = make_clip(1, 16000)
    bits = fx["traj/L64/bits"]
    wm = O.bits_to_bipolar(bits).astype(np.float32)[None]
    batch = rt.Batch([16000])
    dev = net.device_weights(plan)
    sess = rt.EmbedSession(plan, dev, batch, use_graph=True)
    sess.begin(batch.pack([audio]), torch.from_numpy(wm).cuda())
    mine = []
    for _ in range(400):
        sess.iterate(1)
        mine.append(float(sess.loss.cpu()[0]))
    ref = fx["traj/L64/losses"]
    d = np.abs(np.asarray(mine) - ref)
    print(f"L 64: |loss - reference| step0 {d[0]:.2e} first20 {d[:20].max():.2e} max {d.max():.2e} (step {d.argmax()})")
    assert d[0] < 1e-5
    assert d.max() <= 1.6e-2
    out = sess.finish(torch.tensor([float(np.max(audio))], device="cuda"))
    out_c = out.cpu().numpy()
    assert out_c.shape[0] == int(fx["traj/L64/out_len"])
    r = fx["traj/L64/out_sample"]
    rel = np.linalg.norm(out_c[::int(fx["traj/L64/out_step"])] - r) / np.linalg.norm(r)
    print(f"L 64: relative L2 distance to the reference's watermarked audio {rel:.3e}")
    assert rel <= 0.15
    vals = rt.detect(plan, dev, rt.Batch([out_c.shape[0]]), out).cpu().numpy()[0]
    np.testing.assert_array_equal(O.decode_bits(vals), fx["traj/L64/det_bits"])


def test_variant_on_the_staged_route_at_64_bits(rt, plan, O):
    """gelu blocks, batch norm, sigmoid read-out at 64 bits (staged route: wide read-out writes dL/dA): detector entry points
    against the float64 restatement and the first embed gradient with push_sigmoid against float64 autograd."""
    L = 64
    net = make_net(L, activation="gelu", norm_layer="batch", final_activation="sigmoid")
    dev = net.device_weights(plan)
    assert not dev.is_card
    vd = VariantDetector(net)
    for lengths in ([16000] * 32, RAGGED[:4]):
        batch = rt.Batch(lengths)
        rng = np.random.default_rng(3)
        mags = band_mags(rng, batch.frames)
        rows = torch.zeros((batch.total_frames, rt.SPEC_STRIDE), dtype=torch.float32)
        for i, m in enumerate(mags):
            rows[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :225] = torch.from_numpy(m[32:257].T)
        rows = rows.cuda()
        target = torch.from_numpy(payload(9, batch.B, L))
        vals = rt.detector_forward(plan, dev, batch, rows)
        p = vals.detach().clone().requires_grad_(True)
        push_extremes_sum(p, target.cuda()).backward()
        _, gmag = rt.detector_backward(plan, dev, batch, rows, p.grad)
        vals, gmag = vals.cpu().numpy(), gmag.cpu().numpy()
        for i in (0, batch.B - 1):
            x = torch.from_numpy(mags[i]).double()[None].requires_grad_(True)
            ref = vd.forward(x)
            push_extremes_sum(ref, target[i:i + 1].double()).backward()
            np.testing.assert_allclose(vals[i], ref.detach().numpy()[0], atol=5e-5)
            mine = gmag[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :225].T
            check_gradient(mine, x.grad.numpy()[0, 32:257], vd.kink_distance(x.detach())[0], f"staged clip {i}", 1e-4)
    lengths = [16000] * 32
    clips = [make_clip(900 + i, n)[0] for i, n in enumerate(lengths)]
    wm = payload(11, len(lengths), L)
    batch = rt.Batch(lengths)
    sess = rt.EmbedSession(plan, dev, batch, use_graph=False, loss="push_sigmoid")
    sess.begin(batch.pack(clips), torch.from_numpy(wm).cuda())
    g = sess.gradient().cpu().numpy()
    lv = sess.loss.cpu().numpy()
    det64 = VariantDetector(net, torch.float64)
    for i in (0, 31):
        l_ref, _, ref, kink = oracle_first_iteration(O, det64, vd, clips[i], wm[i], "push_sigmoid")
        assert abs(lv[i] - l_ref) < 2e-5, (i, lv[i], l_ref)
        check_gradient(g[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :225].T, ref, kink, f"staged embed clip {i}", 1e-4)


def test_graph_replay_matches_eager_at_64_bits(rt, plan):
    """Graph replay and eager iteration give the same losses and coefficients at 64 bits."""
    L = 64
    dev = make_net(L).device_weights(plan)
    lengths = [16000] * 32
    clips = [make_clip(1000 + i, n)[0] for i, n in enumerate(lengths)]
    wm = torch.from_numpy(payload(13, len(lengths), L)).cuda()
    batch = rt.Batch(lengths)
    res = []
    for graph in (False, True):
        sess = rt.EmbedSession(plan, dev, batch, num_iterations=30, use_graph=graph)
        sess.begin(batch.pack(clips), wm)
        losses = []
        for _ in range(30):
            sess.iterate(1)
            losses.append(sess.loss.cpu().numpy().copy())
        res.append((np.stack(losses), sess.coef.cpu().numpy().copy()))
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])


def test_silent_and_tiny_clips_stay_finite_at_64_bits(rt, plan):
    """A silent clip and a 1e-30-scaled clip inside a 32-clip uniform batch: embed and detect stay finite."""
    L = 64
    dev = make_net(L).device_weights(plan)
    lengths = [16000] * 32
    clips = [make_clip(1100 + i, n)[0] for i, n in enumerate(lengths)]
    clips[3] = np.zeros(16000, np.float32)
    clips[17] = (clips[17] * 1e-30).astype(np.float32)
    wm = torch.from_numpy(payload(17, len(lengths), L)).cuda()
    batch = rt.Batch(lengths)
    sess = rt.EmbedSession(plan, dev, batch, num_iterations=20, use_graph=False)
    sess.begin(batch.pack(clips), wm)
    sess.iterate(20)
    assert bool(torch.isfinite(sess.loss).all())
    assert bool(torch.isfinite(sess.coef).all())
    out = sess.finish(torch.tensor([float(np.max(np.abs(c))) for c in clips], device="cuda"))
    assert bool(torch.isfinite(out).all())
    vals = rt.detect(plan, dev, rt.Batch(batch.out_lengths, in_offsets=batch.out_offsets), out)
    assert tuple(vals.shape) == (32, L)
    assert bool(torch.isfinite(vals).all())


@pytest.mark.parametrize("L", [33, 64])
def test_training_extension_gradients_vs_autograd(rt, plan, O, L):
    """EXTENSION (detector training): dL/dW and dL/db of every block in the caller's shapes ([2L][1024] and [2L] for the last)
    and dL/dmag against torch autograd in float64, on a ragged batch."""
    net = make_net(L)
    dev = net.device_weights(plan)
    lengths = [16000, 24000]
    clips = [make_clip(300 + i, n)[0] for i, n in enumerate(lengths)]
    batch = rt.Batch(lengths)
    x = batch.pack(clips)
    mag, _ = rt.stft_band(plan, batch, x, normalize=True)
    cot = torch.randn(2, L, generator=torch.Generator().manual_seed(L))
    vals, gmag, gw, gb = rt.detector_weight_gradients(plan, dev, batch, mag, cot.cuda())
    torch.cuda.synchronize()
    assert tuple(gw[-1].shape) == (2 * L, 1024) and tuple(gb[-1].shape) == (2 * L,)
    det64 = PayloadDetector(L)
    ws = [w.clone().requires_grad_(True) for w in det64.ws]
    bs = [b.clone().requires_grad_(True) for b in det64.bs]
    det64.ws, det64.bs = ws, bs
    oe = O.Embedder()
    total = 0.0
    for i, c in enumerate(clips):
        a = torch.from_numpy(c)[None]
        m = torch.abs(O.stft(a / torch.amax(torch.abs(a) + 1e-8))).double().clone()
        m[:, oe.nonband] = 0.0
        out = det64.forward(m)
        np.testing.assert_allclose(vals[i].cpu().numpy(), out[0].detach().numpy(), atol=5e-5)
        total = total + (out[0] * cot[i].double()).sum()
    total.backward()
    for l in range(4):
        ref = ws[l].grad
        rel = float((gw[l].cpu().double() - ref).norm() / ref.norm())
        print(f"L {L} layer {l}: dL/dW rel L2 vs autograd {rel:.2e}")
        assert rel < 2e-4, (l, rel)
        assert float(gb[l].abs().max()) < 1e-4 * float(ref.abs().max()) * ref.shape[1]
    assert bool(torch.isfinite(gmag).all())


def test_service_round_trip_with_an_8_byte_payload(rt):
    """embed_watermark / detect_watermark with pattern_mode bytes2bipolar and an 8-byte (64-bit) payload."""
    from aware_amd.detection import AWAREDetector
    from aware_amd.embedding import AWAREEmbedder
    from aware_amd.service import detect_watermark, embed_watermark
    emb = AWAREEmbedder(pattern_mode="bytes2bipolar", detection_net_cfg={"output_length": 64}, loss="push_extremes",
                        verbose=False)
    det = AWAREDetector(model=emb.detection_net, threshold=0.0, pattern_mode="bytes2bipolar")
    payload_bytes = bytes([0xA5, 0x3C, 0x00, 0xFF, 0x12, 0x34, 0x56, 0x78])
    audio, _ = make_clip(21, 48000)
    out = embed_watermark(audio, 16000, payload_bytes, emb)
    assert np.isfinite(out).all()
    got = detect_watermark(out, 16000, det)
    want = np.unpackbits(np.frombuffer(payload_bytes, np.uint8))
    # the reference's bytes2bipolar decoder emits one byte per bit (decoder.py:53-57)
    assert len(got) == 64
    np.testing.assert_array_equal(np.frombuffer(bytes(got), np.uint8), want)
