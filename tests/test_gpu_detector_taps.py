"""GPU tests of detectors with temporal convolutions (detection_net_cfg kernel_size / stride / padding behind the key
temporal_convs): the plug-in seam against the reference, the unfold and fold kernels bit for bit, the
detector entry points and the embed loop's first gradient on every conv pipe against float64, workspace exactness, the
reference's own 400-step embeds, graph replay, the key at 1 / 1 / 0, the card after tap detectors, the general route, a loop
attack, the service and the C ABI's refusals.  Without the feature every one of them fails at AWAREDetectorNet (the key)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, make_clip
from test_detector_taps_host import CONFIGS, KSP, TRAJ, TapDetector, fold_rows, make_net, unfold_rows
from test_detector_variants_host import fixture_magnitudes, push_extremes_sum
from test_general_geometry_host import GeneralLoop
from test_gpu_payload_length import band_mags, check_gradient, oracle_first_iteration, payload

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "detector_taps.npz")
# the batches of the entry-point and embed tests: 32 clips of 1 s, and 0.3, 1, 2.5 and 4 s
BATCHES = {"uniform": ([16000] * 32, [0, 31]), "ragged": ([4800, 16000, 40000, 64000], [0, 1, 2, 3])}
ENTRY = ["k3", "k3_s2", "k3_odd"]
# loss bound of the 400-step trajectories: 1.6e-2 as for the card and the sibling trajectories
TRAJ_LOSS_BOUND = {"k3": 1.6e-2, "k3_s2": 1.6e-2}


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


def card_figures(rt, plan):
    """Detect values and the first embed gradient of the model card's net on 32 clips of 1 s."""
    from aware_amd.detection import AWAREDetectorNet
    dev = AWAREDetectorNet().device_weights(plan)
    lengths = [16000] * 32
    clips = [make_clip(900 + i, n)[0] for i, n in enumerate(lengths)]
    batch = rt.Batch(lengths)
    audio = batch.pack(clips)
    vals = rt.detect(plan, dev, batch, audio).clone()
    sess = rt.EmbedSession(plan, dev, batch, use_graph=False)
    sess.begin(audio, torch.from_numpy(payload(5, 32, 20)).cuda())
    g = sess.gradient().clone()
    torch.cuda.synchronize()
    return vals, g


@pytest.fixture(scope="module", autouse=True)
def card_before(rt, plan):
    """The card's figures before this module creates its first tap detector."""
    return card_figures(rt, plan)


def band_rows(rt, batch, mags):
    rows = torch.zeros((batch.total_frames, rt.SPEC_STRIDE), dtype=torch.float32)
    for i, m in enumerate(mags):
        rows[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :225] = torch.from_numpy(m[32:257].T)
    return rows.cuda()


def pooled_offsets(batch):
    off = [0]
    for t in batch.frames:
        off.append(off[-1] + ((t // 2 + 31) & ~31))
    assert off[-1] == batch.total_pooled
    return off


# ---- the seam against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_forward_and_gradient_vs_reference(rt, fx, name):
    """AWAREDetectorNet.forward and its magnitude gradient (plug-in seam) against the reference's float32 CPU run: the bounds
    of tests/test_gpu_detector_sizes.py (pred 5e-5; gradient 2e-4 relative L2 per clip, 2e-2 with a pre-activation within
    1e-5 of 0 in the float64 model)."""
    net = make_net(name)
    L = net.output_length
    mag = torch.from_numpy(fixture_magnitudes()).cuda().requires_grad_(True)
    pred = net.forward(mag)
    assert tuple(pred.shape) == (2, L, 1)
    err = float(np.max(np.abs(pred.detach().cpu().numpy() - fx[f"net/{name}/pred"])))
    print(f"{name}: pred err {err:.1e} (bound 5e-5)")
    push_extremes_sum(pred, torch.from_numpy(fx[f"net/{name}/target"]).cuda()).backward()
    g = mag.grad.cpu().numpy()[:, 32:257, ::int(fx["grad_step"])]
    kink = TapDetector(net).kink_distance(torch.from_numpy(fixture_magnitudes()).double())
    assert err < 5e-5
    for b in range(g.shape[0]):
        check_gradient(g[b], fx[f"net/{name}/grad"][b], kink[b], f"{name} clip {b}", 2e-4)


# ---- unfold and fold alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s,p", KSP)
def test_unfold_and_fold_bit_for_bit(rt, k, s, p):
    """aware_conv_unfold / aware_conv_fold against the torch statement, bit for bit (every value is a copy or a short ordered
    sum): one ragged batch with 1, 3, 31, 32, 33 and 64 pooled rows -- the 32-row clip ends exactly where the next one
    starts -- on blocks 0 and 1, at two widths.  Every row of the input is non-zero, the padding rows included, so a read
    across a clip's end would show; the outputs start as NaN, so the rows up to each clip's boundary must have been written
    as zeros."""
    lib = rt.load_library()
    lengths = [513, 1536, 15872, 16384, 16896, 32768]
    batch = rt.Batch(lengths)
    assert [t // 2 for t in batch.frames] == [1, 3, 31, 32, 33, 64]
    off = pooled_offsets(batch)
    assert off == [0, 32, 64, 96, 128, 192, 256]
    NP = batch.total_pooled
    g = torch.Generator().manual_seed(1000 * k + 10 * s + p)
    for Cs in (4, 72):
        x = torch.randn(NP, Cs, generator=g) + 3.0
        du = torch.randn(NP, k * Cs, generator=g) + 3.0
        xd, dud = x.cuda(), du.cuda()
        for block in (0, 1):
            u = torch.full((NP, k * Cs), float("nan"), device="cuda")
            dx = torch.full((NP, Cs), float("nan"), device="cuda")
            assert lib.aware_conv_unfold(batch.h, rt._ptr(xd), rt._ptr(u), Cs, block, k, s, p, rt._stream()) == 0
            assert lib.aware_conv_fold(batch.h, rt._ptr(dud), rt._ptr(dx), Cs, block, k, s, p, rt._stream()) == 0
            u, dx = u.cpu(), dx.cpu()
            for b, t in enumerate(batch.frames):
                L_in = lib.aware_conv_rows(t // 2, block, k, s, p)
                L_out = lib.aware_conv_rows(t // 2, block + 1, k, s, p)
                r0, r1 = off[b], off[b + 1]
                want_u = torch.zeros((r1 - r0, k * Cs))
                want_u[:L_out] = unfold_rows(x[r0:r0 + L_in], L_out, k, s, p)
                want_dx = torch.zeros((r1 - r0, Cs))
                want_dx[:L_in] = fold_rows(du[r0:r0 + L_out], L_in, k, s, p)
                assert torch.equal(u[r0:r1], want_u), (k, s, p, Cs, block, b)
                assert torch.equal(dx[r0:r1], want_dx), (k, s, p, Cs, block, b)


# ---- entry points and the embed loop against float64 -------------------------------------------------------------------
@pytest.mark.parametrize("which", list(BATCHES))
@pytest.mark.parametrize("name", ENTRY)
def test_detector_entry_points_vs_float64(rt, plan, O, name, which):
    """aware_detect, aware_detector_forward and aware_detector_backward against the float64 model: values to 5e-5 (detect from
    audio: 1e-4, the bound of the wide-band and general-route tests for the same values), the push_extremes magnitude
    gradient per clip to 1e-4 relative L2 (2e-2 near a kink)."""
    lengths, sample = BATCHES[which]
    net = make_net(name)
    L = net.output_length
    dev = net.device_weights(plan)
    assert not dev.is_card
    kk, ss, pp = C.c_int(), C.c_int(), C.c_int()
    assert dev.lib.aware_detector_conv(dev.h, C.byref(kk), C.byref(ss), C.byref(pp)) == 0
    assert (kk.value, ss.value, pp.value) == (net.kernel_size, net.stride, net.padding)
    batch = rt.Batch(lengths)
    rng = np.random.default_rng(len(lengths) + L)
    mags = band_mags(rng, batch.frames)
    rows = band_rows(rt, batch, mags)
    target = torch.from_numpy(payload(len(lengths), batch.B, L))
    vals = rt.detector_forward(plan, dev, batch, rows)
    p = vals.detach().clone().requires_grad_(True)
    push_extremes_sum(p, target.cuda()).backward()
    vals2, gmag = rt.detector_backward(plan, dev, batch, rows, p.grad)
    clips = [make_clip(500 + i, n)[0] for i, n in enumerate(lengths)]
    heard = rt.detect(plan, dev, batch, batch.pack(clips)).cpu().numpy()
    vals, vals2, gmag = vals.cpu().numpy(), vals2.cpu().numpy(), gmag.cpu().numpy()
    np.testing.assert_array_equal(vals, vals2)
    assert np.isfinite(gmag).all() and np.isfinite(heard).all()
    vd = TapDetector(net)
    emb64 = O.Embedder(dtype=torch.float64)
    emb64.det = vd
    for i in sample:
        x = torch.from_numpy(mags[i]).double()[None].requires_grad_(True)
        ref = vd.forward(x)
        push_extremes_sum(ref, target[i:i + 1].double()).backward()
        href = emb64.detect_raw(torch.from_numpy(clips[i]).double()[None])[0].numpy()
        print(f"{name} clip {i} (T {batch.frames[i]}): forward err {np.max(np.abs(vals[i] - ref.detach().numpy()[0])):.1e}, "
              f"detect err {np.max(np.abs(heard[i] - href)):.1e}")
        np.testing.assert_allclose(vals[i], ref.detach().numpy()[0], atol=5e-5)
        np.testing.assert_allclose(heard[i], href, atol=1e-4)
        mine = gmag[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :225].T
        check_gradient(mine, x.grad.numpy()[0, 32:257], vd.kink_distance(x.detach())[0], f"{name} clip {i} (T {batch.frames[i]})",
                       1e-4)


_FIRST = {}


def first_iteration_reference(O, net, name, which, clips, wm, sample):
    """float64 autograd of the reference-shaped loop's first iteration per sampled clip: computed once, shared by the pipes."""
    if (name, which) not in _FIRST:
        vd = TapDetector(net)
        _FIRST[name, which] = {i: oracle_first_iteration(O, vd, vd, clips[i], wm[i], "push_extremes") for i in sample}
    return _FIRST[name, which]


@pytest.mark.parametrize("pipe", ["f16x2", "f32", "bf16x3"])
@pytest.mark.parametrize("which", list(BATCHES))
@pytest.mark.parametrize("name", ENTRY)
def test_first_embed_gradient_vs_float64(rt, plan, O, name, which, pipe):
    """aware_embed_gradient against float64 autograd of the reference-shaped loop: loss to 2e-5, prediction to 5e-5, dL/dcoef
    per clip to 1e-4 relative L2 (kink-checked), on every conv pipe, uniform and ragged."""
    lengths, sample = BATCHES[which]
    net = make_net(name)
    L = net.output_length
    clips = [make_clip(700 + i, n)[0] for i, n in enumerate(lengths)]
    wm = payload(L + 1, len(lengths), L)
    batch = rt.Batch(lengths)
    sess = rt.EmbedSession(plan, net.device_weights(plan), batch, use_graph=False, conv_pipe=pipe)
    sess.begin(batch.pack(clips), torch.from_numpy(wm).cuda())
    g = sess.gradient().cpu().numpy()
    lv, pv = sess.loss.cpu().numpy(), sess.pred.cpu().numpy()
    refs = first_iteration_reference(O, net, name, which, clips, wm, sample)
    figures = []
    for i in sample:
        l_ref, p_ref, ref, kink = refs[i]
        mine = g[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :225].T
        rel = float(np.linalg.norm(mine - ref) / max(np.linalg.norm(ref), 1e-30))
        print(f"{name} {pipe} clip {i}: loss err {abs(lv[i] - l_ref):.1e}, pred err {np.max(np.abs(pv[i] - p_ref)):.1e}, "
              f"gradient rel L2 {rel:.2e} (kink {kink:.1e})")
        figures.append((i, abs(lv[i] - l_ref), float(np.max(np.abs(pv[i] - p_ref))), mine, ref, kink))
    for i, el, ep, mine, ref, kink in figures:
        assert el < 2e-5, (i, el)
        assert ep < 5e-5, (i, ep)
        check_gradient(mine, ref, kink, f"{name} {pipe} clip {i}", 1e-4)


@pytest.mark.parametrize("name", ["k3", "k3_odd", "k3_gelu_batch_sigmoid"])
def test_workspace_bytes_are_exact(rt, plan, name):
    """aware_detect, aware_detector_backward and aware_embed_create run in exactly the size their *_workspace_bytes reports
    (the unfold scratch counted) and refuse one byte less (AWARE_E_WORKSPACE).  aware_embed_workspace_bytes is the size of the
    longest loop with the L1 term, so the session is created so."""
    from aware_amd._lib import EmbedConfig
    net = make_net(name)
    L = net.output_length
    dev = net.device_weights(plan)
    lengths = [4800, 16000, 40000]
    batch = rt.Batch(lengths)
    lib = plan.lib
    audio = batch.pack([make_clip(i, n)[0] for i, n in enumerate(lengths)])
    rows = band_rows(rt, batch, band_mags(np.random.default_rng(5), batch.frames))
    gv = torch.from_numpy(payload(3, batch.B, L)).cuda()
    vals = torch.empty((batch.B, L), dtype=torch.float32, device="cuda")
    gmag = torch.empty_like(rows)

    def run(nbytes, call):
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        return call(rt._ptr(ws), nbytes - 1), call(rt._ptr(ws), nbytes)

    n = lib.aware_detect_workspace_bytes(batch.h, dev.h)
    assert run(n, lambda ws, nb: lib.aware_detect(plan.h, dev.h, batch.h, rt._ptr(audio), rt._ptr(vals), ws, nb,
                                                  rt._stream())) == (-4, 0)
    n = lib.aware_detector_backward_workspace_bytes(batch.h, dev.h)
    assert run(n, lambda ws, nb: lib.aware_detector_backward(dev.h, batch.h, rt._ptr(rows), rt._ptr(gv), rt._ptr(vals),
                                                             rt._ptr(gmag), ws, nb, rt._stream())) == (-4, 0)
    # the scratch is counted: a detector of the same sizes with 1x1 convolutions needs less
    flat = make_net(name, kernel_size=1, stride=1, padding=0).device_weights(plan)
    assert lib.aware_detect_workspace_bytes(batch.h, flat.h) < lib.aware_detect_workspace_bytes(batch.h, dev.h)
    n = lib.aware_embed_workspace_bytes(batch.h, dev.h)
    cfg = EmbedConfig(4096, 6.0, rt.LOSS_KINDS["push_extremes_l1"], 0.1, 0.9, 0.999, 1e-8, 4e-3, 0, 0, 0, 0, 0.5, 0, 0)
    h = C.c_void_p()
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert lib.aware_embed_create(C.byref(h), plan.h, dev.h, batch.h, C.byref(cfg), rt._ptr(ws), n - 1, rt._stream()) == -4
    assert lib.aware_embed_create(C.byref(h), plan.h, dev.h, batch.h, C.byref(cfg), rt._ptr(ws), n, rt._stream()) == 0
    lib.aware_embed_destroy(h)
    torch.cuda.synchronize()
    assert torch.isfinite(vals).all() and torch.isfinite(gmag).all()


# ---- the reference's own embeds ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TRAJ))
def test_embed_trajectory_400_steps_vs_reference(rt, plan, fx, O, name):
    """The reference's own 400-step embed with an edited card (k3 on the 1 s seed clip, the strided two-block net on the 3 s
    one): every step's loss within 1.6e-2, the watermarked waveform within 0.15 relative L2, the detected bits equal the
    reference's, and BER 0."""
    from aware_amd.detection import AWAREDetectorNet
    n, kw = TRAJ[name]
    net = AWAREDetectorNet(temporal_convs=True, **kw)
    audio, _ = make_clip(1, n)
    bits = fx[f"traj/{name}/bits"]
    wm = O.bits_to_bipolar(bits).astype(np.float32)[None]
    batch = rt.Batch([n])
    dev = net.device_weights(plan)
    sess = rt.EmbedSession(plan, dev, batch, use_graph=True)
    sess.begin(batch.pack([audio]), torch.from_numpy(wm).cuda())
    mine = []
    for _ in range(400):
        sess.iterate(1)
        mine.append(float(sess.loss.cpu()[0]))
    d = np.abs(np.asarray(mine) - fx[f"traj/{name}/losses"])
    out = sess.finish(torch.tensor([float(np.max(audio))], device="cuda"))
    out_c = out.cpu().numpy()
    assert out_c.shape[0] == int(fx[f"traj/{name}/out_len"])
    r = fx[f"traj/{name}/out_sample"]
    rel = np.linalg.norm(out_c[::int(fx[f"traj/{name}/out_step"])] - r) / np.linalg.norm(r)
    vals = rt.detect(plan, dev, rt.Batch([out_c.shape[0]]), out).cpu().numpy()[0]
    print(f"{name}: |loss - reference| step0 {d[0]:.2e} step1 {d[1]:.2e} first20 {d[:20].max():.2e} max {d.max():.2e} "
          f"(step {d.argmax()}); waveform rel L2 {rel:.3e}; values vs reference {np.max(np.abs(vals - fx[f'traj/{name}/raw_marked'])):.2e}")
    np.testing.assert_array_equal(O.decode_bits(vals), fx[f"traj/{name}/det_bits"])
    np.testing.assert_array_equal(np.asarray(O.decode_bits(vals)).reshape(-1), bits)
    assert d[0] < 1e-5
    assert d.max() <= TRAJ_LOSS_BOUND[name]
    assert rel <= 0.15


@pytest.mark.parametrize("name", ["k3_odd", "k3_s2"])
def test_graph_replay_matches_eager_and_runs_repeat(rt, plan, name):
    """Graph replay and eager iteration give the same losses and coefficients bit for bit, and so do two runs."""
    net = make_net(name)
    dev = net.device_weights(plan)
    lengths = [16000] * 32
    clips = [make_clip(1000 + i, n)[0] for i, n in enumerate(lengths)]
    wm = torch.from_numpy(payload(13, len(lengths), net.output_length)).cuda()
    batch = rt.Batch(lengths)
    res = []
    for graph in (False, True, True):
        sess = rt.EmbedSession(plan, dev, batch, num_iterations=30, use_graph=graph)
        sess.begin(batch.pack(clips), wm)
        losses = []
        for _ in range(30):
            sess.iterate(1)
            losses.append(sess.loss.cpu().numpy().copy())
        res.append((np.stack(losses), sess.coef.cpu().numpy().copy()))
    for other in res[1:]:
        np.testing.assert_array_equal(res[0][0], other[0])
        np.testing.assert_array_equal(res[0][1], other[1])
    assert np.isfinite(res[0][0]).all()


def test_the_key_at_1_1_0_changes_nothing(rt, plan):
    """With the key and kernel_size / stride / padding 1 / 1 / 0 the detect values, the first gradient and a 16-step output
    are bit-identical to the same net without the key, and the detector is the card's."""
    from aware_amd.detection import AWAREDetectorNet
    lengths = [16000] * 32
    clips = [make_clip(300 + i, n)[0] for i, n in enumerate(lengths)]
    wm = torch.from_numpy(payload(7, 32, 20)).cuda()
    batch = rt.Batch(lengths)
    audio = batch.pack(clips)
    res = []
    for kw in (dict(), dict(temporal_convs=True, kernel_size=1, stride=1, padding=0)):
        dev = AWAREDetectorNet(**kw).device_weights(plan)
        assert dev.is_card and dev.conv == (1, 1, 0)
        vals = rt.detect(plan, dev, batch, audio).clone()
        sess = rt.EmbedSession(plan, dev, batch, num_iterations=16)
        sess.begin(audio, wm)
        g = sess.gradient().clone()
        sess.begin(audio, wm)
        sess.iterate(16)
        out = sess.finish(torch.ones(32, device="cuda")).clone()
        res.append((vals, g, out))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # the C entry point itself: 1 / 1 / 0 is aware_detector_create_ex
    net = AWAREDetectorNet()
    ex = rt.DetectorWeights(plan, net.mel_basis, net.weights, net.biases, arch=net.architecture())
    cv = rt.DetectorWeights(plan, net.mel_basis, [w[:, :, None] for w in net.weights], net.biases, arch=net.architecture(),
                            conv=(1, 1, 0))
    assert ex.is_card and cv.is_card
    assert torch.equal(rt.detect(plan, ex, batch, audio), rt.detect(plan, cv, batch, audio))
    assert torch.equal(rt.detect(plan, ex, batch, audio), res[0][0])


def test_general_route_k3(rt):
    """k3 with general_geometry=True at 256 / 64 / 256 on four 1 s clips against the float64 model, within the bounds of
    tests/test_gpu_general_geometry.py: detect 1e-4, first loss 5e-5 max(1, |loss|), first gradient relative L2 2e-4 on
    bf16x3 and 2e-3 on f16x2."""
    from aware_amd.detection import AWAREDetector
    from aware_amd.embedding import AWAREEmbedder
    emb = AWAREEmbedder(frame_length=256, hop_length=64, win_length=256, general_geometry=True, temporal_convs=True,
                        verbose=False, loss="push_extremes", use_graph=False,
                        detection_net_cfg={"n_fft": 256, "sample_rate": 16000, "kernel_size": 3})
    det = AWAREDetector(emb.detection_net, frame_length=256, hop_length=64, win_length=256, general_geometry=True)
    lengths = [16000] * 4
    made = [make_clip(320 + i, n) for i, n in enumerate(lengths)]
    clips = [c for c, _ in made]
    wm = np.stack([(2 * b - 1).astype(np.float32) for _, b in made])
    plan = emb._plan(16000)
    batch = emb.make_batch(lengths, 16000)
    dev = emb.detection_net.device_weights(plan)
    assert plan.general and not dev.is_card and batch.frames == [251] * 4
    e64 = GeneralLoop(256, 64, 256, "hann", 16000, (500, 4000), dtype=torch.float64)
    e64.det = TapDetector(emb.detection_net)
    vals = det.detect_batch(clips, 16000).cpu().numpy()
    ref = [e64.first_iteration(torch.from_numpy(c).double()[None], torch.from_numpy(w).double()[None]) for c, w in zip(clips, wm)]
    for i, c in enumerate(clips):
        want = e64.detect_raw(torch.from_numpy(c).double()[None])[0].numpy()
        print(f"general k3 clip {i}: detect err {np.max(np.abs(vals[i] - want)):.1e} (bound 1e-4)")
        assert np.max(np.abs(vals[i] - want)) < 1e-4
    for pipe, bar in (("bf16x3", 2e-4), ("f16x2", 2e-3)):
        sess = rt.EmbedSession(plan, dev, batch, use_graph=False, conv_pipe=pipe)
        sess.begin(batch.pack(clips), torch.from_numpy(wm).cuda())
        g = sess.gradient().cpu().double()
        loss = sess.loss.cpu().numpy()
        for i, (l_ref, _, g_ref) in enumerate(ref):
            r0, r1 = batch.frame_offsets[i], batch.frame_offsets[i + 1]
            gr = g_ref[0].T.contiguous()
            el = abs(float(loss[i]) - float(l_ref[0])) / max(1.0, abs(float(l_ref[0])))
            rel = float((g[r0:r1, :plan.nband] - gr).norm() / gr.norm())
            print(f"general k3 {pipe} clip {i}: loss err {el:.1e} (bound 5e-5), gradient rel L2 {rel:.2e} (bound {bar:.0e})")
            assert el < 5e-5 and rel < bar, (pipe, i, el, rel)


def test_loop_attack_with_k3(rt):
    """k3 with gaussian noise at 10 dB inside the loop: 100 steps run, the outputs are finite and the clean BER is 0 on four
    1 s clips."""
    from aware_amd.detection import AWAREDetector
    from aware_amd.embedding import AWAREEmbedder
    emb = AWAREEmbedder(detection_net_cfg=dict(kernel_size=3), temporal_convs=True, num_iterations=100, verbose=False,
                        loss="push_extremes", loop_attacks=[{"kind": "gaussian_noise", "snr_db": 10.0}])
    det = AWAREDetector(emb.detection_net)
    made = [make_clip(340 + i, 16000) for i in range(4)]
    clips = [c for c, _ in made]
    bits = np.stack([b for _, b in made])
    outs = emb.embed_batch(clips, 16000, (2 * bits - 1).astype(np.float32))
    outs = [o.cpu().numpy() for o in outs]
    assert all(np.isfinite(o).all() for o in outs)
    vals = det.detect_batch(outs, 16000).cpu().numpy()
    assert np.isfinite(vals).all()
    np.testing.assert_array_equal((vals > 0).astype(bits.dtype), bits)


def test_stereo_service_round_trip_with_an_edited_card(rt, tmp_path):
    """load() of a card with kernel_size 3, padding 1 and the key, then embed_watermark / detect_watermark on a stereo clip:
    every channel carries the payload."""
    import yaml
    from aware_amd.service import detect_watermark, embed_watermark
    from aware_amd.utils.models import load, load_model
    with open(load_model._CARD) as f:
        card = yaml.safe_load(f)
    card["detection_net_cfg"] = dict(card["detection_net_cfg"], kernel_size=3, padding=1)
    card["temporal_convs"] = True
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.detection_net.has_taps and emb.detection_net.weights[0].shape == (512, 128, 3)
    rng = np.random.default_rng(29)
    bits = rng.integers(0, 2, 20).astype(np.int32)
    stereo = np.column_stack([make_clip(51, 32000)[0], make_clip(52, 32000)[0]])
    out = embed_watermark(stereo, 16000, bits, emb)
    assert out.shape[1] == 2 and np.isfinite(out).all()
    got = detect_watermark(out, 16000, det)
    for ch in (got if isinstance(got, (list, tuple)) else [got]):
        np.testing.assert_array_equal(np.asarray(ch).reshape(-1)[:20].astype(np.int32), bits)


def test_c_abi_refusals(rt, plan):
    """aware_detector_create_conv outside the limits (AWARE_E_UNSUPPORTED; non-positive sizes AWARE_E_BADARG), a batch with a
    clip too short for the blocks (AWARE_E_BADARG from aware_detect, aware_detector_forward / _backward and
    aware_embed_create, nothing launched; ValueError from the wrappers), and the training extension (AWARE_E_UNSUPPORTED)."""
    net = make_net("k3")
    lib = plan.lib
    from aware_amd._lib import DetectorArch
    nl = len(net.weights)
    mel = np.ascontiguousarray(net.mel_basis, np.float32)
    big = [np.zeros((w.shape[0], w.shape[1], 8), np.float32) for w in net.weights]       # room for any kernel_size tried
    wp = (C.c_void_p * nl)(*[w.ctypes.data for w in big])
    bp = (C.c_void_p * nl)(*[np.ascontiguousarray(b).ctypes.data for b in net.biases])
    arch = DetectorArch(1, 0, 4, None, None)
    for conv, rc in (((8, 1, 0), -2), ((3, 5, 0), -2), ((3, 1, 2), -2), ((2, 1, 1), -2), ((0, 1, 0), -1), ((3, 0, 0), -1),
                     ((3, 1, -1), -1)):
        h = C.c_void_p()
        assert lib.aware_detector_create_conv(C.byref(h), plan.h, C.c_void_p(mel.ctypes.data), mel.shape[0], nl,
                                              (C.c_int * (nl + 1))(*net.channels), wp, bp, C.byref(arch), *conv) == rc, conv
        assert not h.value
    with pytest.raises(Exception, match="unsupported"):
        rt.DetectorWeights(plan, net.mel_basis, [w[:, :, :3] for w in big], net.biases, arch=net.architecture(), conv=(3, 5, 0))
    dev = net.device_weights(plan)
    batch = rt.Batch([16000, 4100])                      # the second clip: 8 pooled rows, none left behind the fourth block
    assert [t // 2 for t in batch.frames] == [31, 8]
    audio = batch.pack([make_clip(1, 16000)[0], make_clip(2, 4100)[0]])
    rows = torch.zeros((batch.total_frames, rt.SPEC_STRIDE), device="cuda")
    vals = torch.full((2, 20), 7.0, device="cuda")
    gmag = torch.full_like(rows, 7.0)
    n = max(lib.aware_detect_workspace_bytes(batch.h, dev.h), lib.aware_detector_backward_workspace_bytes(batch.h, dev.h))
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert lib.aware_detect(plan.h, dev.h, batch.h, rt._ptr(audio), rt._ptr(vals), rt._ptr(ws), n, rt._stream()) == -1
    assert lib.aware_detector_forward(dev.h, batch.h, rt._ptr(rows), rt._ptr(vals), rt._ptr(ws), n, rt._stream()) == -1
    assert lib.aware_detector_backward(dev.h, batch.h, rt._ptr(rows), rt._ptr(vals), rt._ptr(vals), rt._ptr(gmag), rt._ptr(ws), n,
                                       rt._stream()) == -1
    good = rt.EmbedSession(plan, dev, rt.Batch([16000]), num_iterations=2, use_graph=False)
    big = torch.empty(lib.aware_embed_workspace_bytes(batch.h, dev.h), dtype=torch.uint8, device="cuda")
    h = C.c_void_p()
    assert lib.aware_embed_create(C.byref(h), plan.h, dev.h, batch.h, C.byref(good.cfg), rt._ptr(big), big.numel(),
                                  rt._stream()) == -1
    torch.cuda.synchronize()
    assert float(vals.min()) == 7.0 and float(gmag.min()) == 7.0          # nothing was launched
    for call in (lambda: rt.detect(plan, dev, batch, audio), lambda: rt.detector_forward(plan, dev, batch, rows),
                 lambda: rt.detector_backward(plan, dev, batch, rows, vals), lambda: rt.EmbedSession(plan, dev, batch)):
        with pytest.raises(ValueError, match="clip 1 has 8 pooled rows"):
            call()
    # training: the extension serves the card only
    ws_h = [np.ascontiguousarray(w) for w in net.weights]
    wp = (C.c_void_p * len(ws_h))(*[w.ctypes.data for w in ws_h])
    bp = (C.c_void_p * len(ws_h))(*[np.ascontiguousarray(b).ctypes.data for b in net.biases])
    mel = np.ascontiguousarray(net.mel_basis, np.float32)
    assert lib.aware_detector_update(dev.h, C.c_void_p(mel.ctypes.data), wp, bp) == -2
    one = rt.Batch([16000])
    mag = torch.zeros((one.total_frames, rt.SPEC_STRIDE), device="cuda")
    tn = lib.aware_detector_train_workspace_bytes(one.h, dev.h)
    tws = torch.empty(tn, dtype=torch.uint8, device="cuda")
    loss = torch.empty(1, device="cuda")
    gw = [torch.empty(w.shape, device="cuda") for w in net.weights]
    pw = (C.c_void_p * len(gw))(*[t.data_ptr() for t in gw])
    assert lib.aware_detector_train_gradients(dev.h, one.h, rt._ptr(mag), rt._ptr(vals), 0, rt._ptr(loss), rt._ptr(vals), None, pw,
                                              None, rt._ptr(tws), tn, rt._stream()) == -2
    with pytest.raises(NotImplementedError):
        rt.detector_weight_gradients(plan, dev, one, mag, torch.zeros((1, 20), device="cuda"))


def test_the_card_after_tap_detectors(rt, plan, card_before):
    """After tap detectors have lived in the process, the card's detect values and first gradient are bit-identical to what
    they were before this module made its first one."""
    make_net("k3").device_weights(plan)                  # (at least one, whatever ran before)
    vals, g = card_figures(rt, plan)
    assert torch.equal(vals, card_before[0]) and torch.equal(g, card_before[1])
