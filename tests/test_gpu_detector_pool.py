"""GPU tests of detectors with any initial pool (detection_net_cfg initial_pool_size / initial_pool_stride behind the key
initial_pools): the plug-in seam against the reference, the pool kernels at their edges against float64,
the detector entry points and the embed loop's first gradient on every conv pipe, workspace exactness, the reference's own
400-step embeds, graph replay, the key at (2, 2), the card after pooled detectors, the general route, a loop attack, the
service and the C ABI's refusals.  Without the feature every one of them fails at AWAREDetectorNet (the key)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, make_clip
from test_detector_pool_host import CONFIGS, TRAJ, PoolDetector, make_net, pool
from test_detector_variants_host import fixture_magnitudes, push_extremes_sum
from test_general_geometry_host import GeneralLoop
from test_gpu_detector_taps import BATCHES, band_rows, card_figures
from test_gpu_payload_length import band_mags, check_gradient, oracle_first_iteration, payload

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "detector_pool.npz")
ENTRY = ["p44", "p32", "p44_k3"]
# the pools and banks of the kernels' edge test
EDGE_POOLS = [(4, 4), (3, 2), (2, 3), (3, 3), (8, 2), (8, 8)]
EDGE_BANKS = [128, 80, 200]
# loss bound of the 400-step trajectories: 1.6e-2 as for the card and the sibling trajectories
TRAJ_LOSS_BOUND = 1.6e-2


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


@pytest.fixture(scope="module", autouse=True)
def card_before(rt, plan):
    """The card's figures before this module creates its first pooled detector."""
    return card_figures(rt, plan)


def reported_pool(dev):
    size, stride = C.c_int(), C.c_int()
    assert dev.lib.aware_detector_pool(dev.h, C.byref(size), C.byref(stride)) == 0
    return size.value, stride.value


# ---- 1. the seam against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_forward_and_gradient_vs_reference(rt, fx, name):
    """AWAREDetectorNet.forward and its magnitude gradient (plug-in seam) against the reference's float32 CPU run: pred 5e-5;
    gradient 2e-4 relative L2 per clip, 2e-2 with a pre-activation within 1e-5 of 0 in the float64 model."""
    net = make_net(name)
    L = net.output_length
    mag = torch.from_numpy(fixture_magnitudes()).cuda().requires_grad_(True)
    pred = net.forward(mag)
    assert tuple(pred.shape) == (2, L, 1)
    err = float(np.max(np.abs(pred.detach().cpu().numpy() - fx[f"net/{name}/pred"])))
    print(f"{name}: pred err {err:.1e} (bound 5e-5)")
    push_extremes_sum(pred, torch.from_numpy(fx[f"net/{name}/target"]).cuda()).backward()
    g = mag.grad.cpu().numpy()[:, 32:257, ::int(fx["grad_step"])]
    kink = PoolDetector(net).kink_distance(torch.from_numpy(fixture_magnitudes()).double())
    assert err < 5e-5
    for b in range(g.shape[0]):
        check_gradient(g[b], fx[f"net/{name}/grad"][b], kink[b], f"{name} clip {b}", 2e-4)


# ---- 2. the pool kernels at their edges --------------------------------------------------------------------------------
def edge_frames(size, stride):
    """The clips of one ragged batch, in frames: one row (T = size; a batch holds no clip of fewer than 3 frames); size + 1;
    the longest dropped tail ((T - size) % stride == stride - 1); windows across the 32-frame chunk boundary; exactly 32 rows
    (T = 31 stride + size) with another clip behind it."""
    return [max(size, 3), size + 1, size + 4 * stride - 1, 32, 33, 64, 65, 31 * stride + size, 33]


@pytest.mark.parametrize("n_mels", EDGE_BANKS)
@pytest.mark.parametrize("size,stride", EDGE_POOLS)
def test_pool_kernels_at_their_edges(rt, plan, size, stride, n_mels):
    """aware_detector_forward / _backward of a one-block net (no norm, GELU: no kink, and a block of one row is not
    normalised to zero) against the float64 restatement: values to 5e-5, the push_extremes magnitude gradient per clip to 1e-4
    relative L2 (the clip whose one window covers it has the exact gradient 0 and a bound of its own, below).
    Every call runs on a workspace of NaN and on one of zeros: the results are finite and bit-identical, so no row or
    partial is read that the call did not write."""
    from aware_amd.detection import AWAREDetectorNet
    net = AWAREDetectorNet(n_mels=n_mels, num_blocks=0, n_filters=[], norm_layer="none", activation="gelu", initial_pools=True,
                           **pool(size, stride))
    L = net.output_length
    dev = net.device_weights(plan)
    assert not dev.is_card and reported_pool(dev) == (size, stride)
    frames = edge_frames(size, stride)
    assert (frames[2] - size) % stride == stride - 1 and rt.pool_rows(frames[7], size, stride) == 32
    batch = rt.Batch([256 * (t - 1) + 1 for t in frames])
    assert batch.frames == frames
    lib = plan.lib
    rng = np.random.default_rng(100 * size + 10 * stride + n_mels)
    mags = band_mags(rng, batch.frames)
    rows = band_rows(rt, batch, mags)
    target = torch.from_numpy(payload(size + stride, batch.B, L))
    nf = lib.aware_detect_workspace_bytes(batch.h, dev.h)
    nb = lib.aware_detector_backward_workspace_bytes(batch.h, dev.h)
    runs = []
    for fill in (0xFF, 0x00):                       # all-ones bytes: every float of the workspace is a NaN
        ws = torch.full((max(nf, nb),), fill, dtype=torch.uint8, device="cuda")
        vals = torch.full((batch.B, L), float("nan"), device="cuda")
        assert lib.aware_detector_forward(dev.h, batch.h, rt._ptr(rows), rt._ptr(vals), rt._ptr(ws), nf, rt._stream()) == 0
        p = vals.detach().clone().requires_grad_(True)
        push_extremes_sum(p, target.cuda()).backward()
        ws.fill_(fill)
        vals2 = torch.full_like(vals, float("nan"))
        gmag = torch.full_like(rows, float("nan"))
        gv = p.grad.contiguous()
        assert lib.aware_detector_backward(dev.h, batch.h, rt._ptr(rows), rt._ptr(gv), rt._ptr(vals2), rt._ptr(gmag), rt._ptr(ws),
                                           nb, rt._stream()) == 0
        torch.cuda.synchronize()
        runs.append((vals.cpu().numpy(), vals2.cpu().numpy(), gmag.cpu().numpy()))
    for a, b in zip(*runs):
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, b)
    vals, vals2, gmag = runs[0]
    np.testing.assert_array_equal(vals, vals2)
    vd, vd32 = PoolDetector(net), PoolDetector(net, dtype=torch.float32)
    for i, t in enumerate(frames):
        x = torch.from_numpy(mags[i]).double()[None].requires_grad_(True)
        ref = vd.forward(x)
        push_extremes_sum(ref, target[i:i + 1].double()).backward()
        err = float(np.max(np.abs(vals[i] - ref.detach().numpy()[0])))
        mine = gmag[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :225].T
        want = x.grad.numpy()[0, 32:257]
        assert np.isfinite(mine).all()
        if t == size:
            # One window over the whole clip: the pooled row is the mean of the InstanceNorm's output, identically 0, so the
            # exact gradient is 0 and a relative bound has no denominator.  What is left in float32 is the rounding of terms
            # that cancel; the float32 CPU restatement leaves its own on the same input, and four times its distance to
            # float64 (another summation order, the GEMMs' split arithmetic) is the bound.
            x32 = torch.from_numpy(mags[i])[None].requires_grad_(True)
            push_extremes_sum(vd32.forward(x32), target[i:i + 1]).backward()
            e32 = float(np.linalg.norm(x32.grad.numpy()[0, 32:257] - want))
            mine_err = float(np.linalg.norm(mine - want))
            print(f"pool ({size}, {stride}) n_mels {n_mels} clip {i} (T {t}, 1 row over the whole clip): value err {err:.1e}, "
                  f"|gradient| float64 {np.linalg.norm(want):.1e}, float32 restatement {e32:.2e}, kernels {mine_err:.2e}")
            assert np.linalg.norm(want) < 1e-12 and err < 5e-5 and mine_err <= 4 * e32, (i, t, err, mine_err, e32)
            continue
        rel = float(np.linalg.norm(mine - want) / np.linalg.norm(want))
        print(f"pool ({size}, {stride}) n_mels {n_mels} clip {i} (T {t}, {rt.pool_rows(t, size, stride)} rows): value err "
              f"{err:.1e}, gradient rel L2 {rel:.2e}")
        assert err < 5e-5 and rel < 1e-4, (i, t, err, rel)


# ---- 3. entry points and the embed loop against float64 ----------------------------------------------------------------
@pytest.mark.parametrize("which", list(BATCHES))
@pytest.mark.parametrize("name", ENTRY)
def test_detector_entry_points_vs_float64(rt, plan, O, name, which):
    """aware_detect, aware_detector_forward and aware_detector_backward against the float64 model: values to 5e-5 (detect from
    audio: 1e-4), the push_extremes magnitude gradient per clip to 1e-4 relative L2 (2e-2 near a kink)."""
    lengths, sample = BATCHES[which]
    net = make_net(name)
    L = net.output_length
    dev = net.device_weights(plan)
    assert not dev.is_card and reported_pool(dev) == net.pool and dev.pool == net.pool
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
    vd = PoolDetector(net)
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
        vd = PoolDetector(net)
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


# ---- 4. workspace bytes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p44", "p33_small", "p44_k3"])
def test_workspace_bytes_are_exact(rt, plan, name):
    """aware_detect, aware_detector_backward and aware_embed_create run in exactly the size their *_workspace_bytes reports
    and refuse one byte less (AWARE_E_WORKSPACE); the pool changes no workspace rule, so a staged net of the same sizes after
    the (2, 2) pool reports the same bytes."""
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
    if not make_net(name, initial_pool_size=2, initial_pool_stride=2).is_card_arch:
        same = make_net(name, initial_pool_size=2, initial_pool_stride=2).device_weights(plan)
        for fn in (lib.aware_detect_workspace_bytes, lib.aware_detector_backward_workspace_bytes, lib.aware_embed_workspace_bytes):
            assert fn(batch.h, same.h) == fn(batch.h, dev.h)
    n = lib.aware_embed_workspace_bytes(batch.h, dev.h)
    cfg = EmbedConfig(4096, 6.0, rt.LOSS_KINDS["push_extremes_l1"], 0.1, 0.9, 0.999, 1e-8, 4e-3, 0, 0, 0, 0, 0.5, 0, 0)
    h = C.c_void_p()
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert lib.aware_embed_create(C.byref(h), plan.h, dev.h, batch.h, C.byref(cfg), rt._ptr(ws), n - 1, rt._stream()) == -4
    assert lib.aware_embed_create(C.byref(h), plan.h, dev.h, batch.h, C.byref(cfg), rt._ptr(ws), n, rt._stream()) == 0
    lib.aware_embed_destroy(h)
    torch.cuda.synchronize()
    assert torch.isfinite(vals).all() and torch.isfinite(gmag).all()


# ---- 5. the reference's own embeds -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TRAJ))
def test_embed_trajectory_400_steps_vs_reference(rt, plan, fx, O, name):
    """The reference's own 400-step embed with an edited card (p44 on the 1 s seed clip, the overlapping (3, 2) pool on the
    3 s one): every step's loss within 1.6e-2, the watermarked waveform within 0.15 relative L2, the detected bits equal the
    reference's (which read its own payload back: BER 0)."""
    from aware_amd.detection import AWAREDetectorNet
    n, kw = TRAJ[name]
    net = AWAREDetectorNet(initial_pools=True, **kw)
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
    assert d.max() <= TRAJ_LOSS_BOUND
    assert rel <= 0.15


# ---- 6. graph replay and repeats ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p32", "p44_k3"])
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


# ---- 7. the key at (2, 2) ----------------------------------------------------------------------------------------------
def test_the_key_at_2_2_changes_nothing(rt, plan):
    """With the key and the (2, 2) pool the detect values, the first gradient, five losses and the embedded output are
    bit-identical to the same net without the key, and the detector is the card's."""
    from aware_amd.detection import AWAREDetectorNet
    lengths = [16000] * 32
    clips = [make_clip(300 + i, n)[0] for i, n in enumerate(lengths)]
    wm = torch.from_numpy(payload(7, 32, 20)).cuda()
    batch = rt.Batch(lengths)
    audio = batch.pack(clips)
    res = []
    for kw in (dict(), dict(initial_pools=True, **pool(2, 2))):
        dev = AWAREDetectorNet(**kw).device_weights(plan)
        assert dev.is_card and dev.pool == (2, 2) and reported_pool(dev) == (2, 2)
        vals = rt.detect(plan, dev, batch, audio).clone()
        sess = rt.EmbedSession(plan, dev, batch, num_iterations=16)
        sess.begin(audio, wm)
        g = sess.gradient().clone()
        sess.begin(audio, wm)
        losses = []
        for _ in range(5):
            sess.iterate(1)
            losses.append(sess.loss.clone())
        sess.iterate(11)
        out = sess.finish(torch.ones(32, device="cuda")).clone()
        res.append((vals, g, torch.stack(losses), out))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # the C entry point itself: 2 / 2 is aware_detector_create_conv, and 1 / 1 / 0 there aware_detector_create_ex
    net = AWAREDetectorNet()
    ex = rt.DetectorWeights(plan, net.mel_basis, net.weights, net.biases, arch=net.architecture())
    pl = rt.DetectorWeights(plan, net.mel_basis, net.weights, net.biases, arch=net.architecture(), pool=(2, 2))
    assert ex.is_card and pl.is_card and reported_pool(ex) == (2, 2) and reported_pool(pl) == (2, 2)
    assert torch.equal(rt.detect(plan, ex, batch, audio), rt.detect(plan, pl, batch, audio))
    assert torch.equal(rt.detect(plan, ex, batch, audio), res[0][0])
    # every older way of making a detector reports 2 / 2
    old = rt.DetectorWeights(plan, net.mel_basis, net.weights, net.biases)
    assert reported_pool(old) == (2, 2)


# ---- 8. other routes, one each -----------------------------------------------------------------------------------------
def test_general_route_p44(rt):
    """p44 with general_geometry=True at 256 / 64 / 256 on four 1 s clips against the float64 model, within the bounds of
    tests/test_gpu_general_geometry.py: detect 1e-4, first loss 5e-5 max(1, |loss|), first gradient relative L2 2e-4 on
    bf16x3 and 2e-3 on f16x2."""
    from aware_amd.detection import AWAREDetector
    from aware_amd.embedding import AWAREEmbedder
    emb = AWAREEmbedder(frame_length=256, hop_length=64, win_length=256, general_geometry=True, initial_pools=True,
                        verbose=False, loss="push_extremes", use_graph=False,
                        detection_net_cfg=dict({"n_fft": 256, "sample_rate": 16000}, **pool(4, 4)))
    det = AWAREDetector(emb.detection_net, frame_length=256, hop_length=64, win_length=256, general_geometry=True)
    lengths = [16000] * 4
    made = [make_clip(320 + i, n) for i, n in enumerate(lengths)]
    clips = [c for c, _ in made]
    wm = np.stack([(2 * b - 1).astype(np.float32) for _, b in made])
    plan = emb._plan(16000)
    batch = emb.make_batch(lengths, 16000)
    dev = emb.detection_net.device_weights(plan)
    assert plan.general and not dev.is_card and batch.frames == [251] * 4 and reported_pool(dev) == (4, 4)
    e64 = GeneralLoop(256, 64, 256, "hann", 16000, (500, 4000), dtype=torch.float64)
    e64.det = PoolDetector(emb.detection_net)
    vals = det.detect_batch(clips, 16000).cpu().numpy()
    ref = [e64.first_iteration(torch.from_numpy(c).double()[None], torch.from_numpy(w).double()[None]) for c, w in zip(clips, wm)]
    for i, c in enumerate(clips):
        want = e64.detect_raw(torch.from_numpy(c).double()[None])[0].numpy()
        print(f"general p44 clip {i}: detect err {np.max(np.abs(vals[i] - want)):.1e} (bound 1e-4)")
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
            print(f"general p44 {pipe} clip {i}: loss err {el:.1e} (bound 5e-5), gradient rel L2 {rel:.2e} (bound {bar:.0e})")
            assert el < 5e-5 and rel < bar, (pipe, i, el, rel)


def test_loop_attack_with_p44(rt):
    """p44 with gaussian noise at 10 dB inside the loop: 100 steps run, the outputs are finite, and the clean read of the four
    1 s clips has the bit errors the same net reads after 100 steps without the attack."""
    from aware_amd.detection import AWAREDetector
    from aware_amd.embedding import AWAREEmbedder
    made = [make_clip(340 + i, 16000) for i in range(4)]
    clips = [c for c, _ in made]
    bits = np.stack([b for _, b in made])
    errors = []
    for attacks in ([{"kind": "gaussian_noise", "snr_db": 10.0}], None):
        emb = AWAREEmbedder(detection_net_cfg=pool(4, 4), initial_pools=True, num_iterations=100, verbose=False,
                            loss="push_extremes", loop_attacks=attacks)
        det = AWAREDetector(emb.detection_net)
        outs = [o.cpu().numpy() for o in emb.embed_batch(clips, 16000, (2 * bits - 1).astype(np.float32))]
        assert all(np.isfinite(o).all() for o in outs)
        vals = det.detect_batch(outs, 16000).cpu().numpy()
        assert np.isfinite(vals).all()
        errors.append(int(np.sum((vals > 0).astype(bits.dtype) != bits)))
    print(f"p44, 100 steps: bit errors with the attack in the loop {errors[0]}, without {errors[1]}")
    assert errors[0] == errors[1]


def test_stereo_service_round_trip_with_an_edited_card(rt, tmp_path):
    """load() of a card with the (4, 4) pool and the key, then embed_watermark / detect_watermark on a stereo clip: every
    channel carries the payload."""
    import yaml
    from aware_amd.service import detect_watermark, embed_watermark
    from aware_amd.utils.models import load, load_model
    with open(load_model._CARD) as f:
        card = yaml.safe_load(f)
    card["detection_net_cfg"] = dict(card["detection_net_cfg"], **pool(4, 4))
    card["initial_pools"] = True
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.detection_net.has_pool and emb.detection_net.pool == (4, 4)
    rng = np.random.default_rng(29)
    bits = rng.integers(0, 2, 20).astype(np.int32)
    stereo = np.column_stack([make_clip(51, 32000)[0], make_clip(52, 32000)[0]])
    out = embed_watermark(stereo, 16000, bits, emb)
    assert out.shape[1] == 2 and np.isfinite(out).all()
    got = detect_watermark(out, 16000, det)
    for ch in (got if isinstance(got, (list, tuple)) else [got]):
        np.testing.assert_array_equal(np.asarray(ch).reshape(-1)[:20].astype(np.int32), bits)


# ---- 9. C ABI refusals -------------------------------------------------------------------------------------------------
def test_c_abi_refusals(rt, plan):
    """aware_detector_create_pool outside the range (AWARE_E_UNSUPPORTED; non-positive sizes AWARE_E_BADARG) and on a general
    plan made for the transforms alone, with pointers that are never dereferenced since the refusal comes first; a batch with
    a clip of fewer frames than the pool (AWARE_E_BADARG from aware_detect, aware_detector_forward / _backward and
    aware_embed_create, nothing launched; ValueError from the wrappers); the training extension (AWARE_E_UNSUPPORTED)."""
    net = make_net("p88")
    lib = plan.lib
    from aware_amd._lib import DetectorArch
    nl = len(net.weights)
    never = C.c_void_p(8)                                # not null, never dereferenced
    arch = DetectorArch(1, 0, 4, None, None)
    chans = (C.c_int * (nl + 1))(*net.channels)
    nowhere = C.cast(never, C.POINTER(C.c_void_p))
    for pl, rc in (((9, 2), -2), ((2, 9), -2), ((1, 2), -2), ((2, 1), -2), ((1, 1), -2), ((0, 2), -1), ((2, 0), -1),
                   ((-4, 4), -1), ((4, -4), -1)):
        h = C.c_void_p()
        assert lib.aware_detector_create_pool(C.byref(h), plan.h, never, 128, nl, chans, nowhere, nowhere, C.byref(arch),
                                              1, 1, 0, *pl) == rc, pl
        assert not h.value
    # the conv arguments keep their own refusals behind a served pool
    for conv, rc in (((8, 1, 0), -2), ((0, 1, 0), -1)):
        h = C.c_void_p()
        assert lib.aware_detector_create_pool(C.byref(h), plan.h, never, 128, nl, chans, nowhere, nowhere, C.byref(arch),
                                              *conv, 4, 4) == rc, conv
    with pytest.raises(Exception, match="unsupported"):
        rt.DetectorWeights(plan, net.mel_basis, net.weights, net.biases, arch=net.architecture(), pool=(9, 2))
    # a general plan made for the transforms alone: as for its siblings
    gplan = rt.Plan(256, 64, 256, "hann", band_bins=(8, 64))
    assert gplan.general
    h = C.c_void_p()
    assert lib.aware_detector_create_pool(C.byref(h), gplan.h, never, 128, nl, chans, nowhere, nowhere, C.byref(arch), 1, 1, 0,
                                          4, 4) == -2
    assert not h.value
    dev = net.device_weights(plan)
    batch = rt.Batch([16000, 1791])                      # the second clip: 7 frames, fewer than the pool's 8
    assert batch.frames == [63, 7]
    audio = batch.pack([make_clip(1, 16000)[0], make_clip(2, 1791)[0]])
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
        with pytest.raises(ValueError, match="clip 1 has 7 frames, and the initial pool"):
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
    tws = torch.empty(max(tn, 1), dtype=torch.uint8, device="cuda")
    loss = torch.empty(1, device="cuda")
    gw = [torch.empty(w.shape, device="cuda") for w in net.weights]
    pw = (C.c_void_p * len(gw))(*[t.data_ptr() for t in gw])
    assert lib.aware_detector_train_gradients(dev.h, one.h, rt._ptr(mag), rt._ptr(vals), 0, rt._ptr(loss), rt._ptr(vals), None, pw,
                                              None, rt._ptr(tws), tn, rt._stream()) == -2
    with pytest.raises(NotImplementedError):
        rt.detector_weight_gradients(plan, dev, one, mag, torch.zeros((1, 20), device="cuda"))


def test_the_card_after_pooled_detectors(rt, plan, card_before):
    """After pooled detectors have lived in the process, the card's detect values and first gradient are bit-identical to
    what they were before this module made its first one."""
    make_net("p44").device_weights(plan)                 # (at least one, whatever ran before)
    vals, g = card_figures(rt, plan)
    assert torch.equal(vals, card_before[0]) and torch.equal(g, card_before[1])
