"""Embedding bands of the wide layout (any band inside bins 0..512, rows of 576 floats): the band STFT, the detector, the
embed loop's first gradient on every kernel path, the service entry points with an edited model card, degenerate clips,
and the training extension's refusal.  The reference's mask is freqs >= lo & freqs <= hi on the 513 bins of n_fft 1024,
so [0, 8000] Hz at 16 kHz is every bin, DC and Nyquist included.

Run on the MI355X box:  python -m pytest tests/test_gpu_wide_band.py -m gpu -q -s
"""
import os
import tempfile

import numpy as np
import pytest
import torch

from conftest import make_clip

pytestmark = pytest.mark.gpu

# (20, 448) = [300, 7000] Hz, (64, 384) = [1000, 6000] Hz, (0, 512) = [0, 8000] Hz; (1, 511): every bin but the two real
# ones; (256, 512): the upper half, Nyquist included
BANDS = [(0, 512), (1, 511), (20, 448), (64, 384), (256, 512)]
KINK_REL = 5e-7           # as tests/test_gpu_conv_scales.py: within rounding of a LeakyReLU kink, relative to the layer


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


_PLANS, _DETS = {}, {}


def _plan(rt, band):
    if band not in _PLANS:
        _PLANS[band] = rt.Plan(band_bins=band)
    return _PLANS[band]


def _det(rt, O, band):
    if band not in _DETS:
        ws, bs = O.detector_weights()
        _DETS[band] = rt.DetectorWeights(_plan(rt, band), O.mel_filter_bank(), [w.numpy() for w in ws], [b.numpy() for b in bs])
    return _DETS[band]


def _mask(band):
    k = np.arange(513)
    return (k >= band[0]) & (k <= band[1])


def test_plan_band_stride(rt):
    """Every band of the issue builds a plan with the wide layout; the model card's band keeps the narrow one."""
    assert rt.Plan().band_stride == rt.SPEC_STRIDE == 256
    assert rt.Plan(band_bins=(1, 256)).band_stride == 256
    assert rt.Plan(band_bins=(256, 511)).band_stride == 256
    for band in BANDS:
        assert _plan(rt, band).band_stride == rt.SPEC_STRIDE_WIDE == 576, band
    assert rt.Plan(band_bins=(0, 0)).band_stride == 576          # DC alone
    assert rt.Plan(band_bins=(512, 512)).band_stride == 576      # Nyquist alone


@pytest.mark.parametrize("band", BANDS)
def test_stft_band_matches_torch(rt, band):
    """aware_stft_band (streaming kernels) against torch.stft in float64: magnitude and unit phasor of every band column
    (DC / Nyquist phasors are (+-1, 0): torch.angle gives 0 or pi), zero tail."""
    lengths = [16000, 23456, 48000]
    clips = [make_clip(70 + i, n)[0] for i, n in enumerate(lengths)]
    plan = _plan(rt, band)
    batch = rt.Batch(lengths)
    mag, ph = rt.stft_band(plan, batch, batch.pack(clips), normalize=True)
    torch.cuda.synchronize()
    mag, ph = mag.cpu(), ph.cpu()
    lo, hi = band
    nb = hi - lo + 1
    win = torch.hann_window(1024, dtype=torch.float64)
    for i, c in enumerate(clips):
        x = torch.from_numpy(c).double()
        x = x / (x.abs().max() + 1e-8)
        S = torch.stft(x, 1024, 256, window=win, center=True, return_complex=True)[lo:hi + 1].T     # [T, nb]
        r0, r1 = batch.frame_offsets[i], batch.frame_offsets[i + 1]
        m = mag[r0:r1, :nb].double()
        ref = S.abs()
        assert float((m - ref).abs().max()) < 2e-5 * float(ref.abs().max()), (band, i)
        assert float(mag[r0:r1, nb:].abs().max()) == 0.0
        sig = ref > 1e-3 * ref.max()
        u = ph[r0:r1, :nb].to(torch.complex128)
        uref = S / S.abs().clamp_min(1e-300)
        assert float((u - uref).abs()[sig].max()) < 1e-3, (band, i)
        for k in (0, 512):
            if lo <= k <= hi:
                col = ph[r0:r1, k - lo]
                assert float(col.imag.abs().max()) == 0.0
                assert torch.allclose(col.real.abs(), torch.ones(r1 - r0), atol=1e-6)


def _oracle_detector(O, dtype=torch.float64):
    return O.Detector(dtype)


@pytest.mark.parametrize("band", BANDS)
def test_detector_forward_backward(rt, O, band):
    """aware_detector_forward / _backward on a band of the wide layout against float64 autograd of the oracle network."""
    lengths = [48000] * 4
    clips = [make_clip(80 + i, n)[0] for i, n in enumerate(lengths)]
    plan, det = _plan(rt, band), _det(rt, O, band)
    batch = rt.Batch(lengths)
    mag, _ = rt.stft_band(plan, batch, batch.pack(clips), normalize=True)
    gv = torch.from_numpy(np.random.default_rng(5).standard_normal((4, 20)).astype(np.float32)).cuda()
    vals = rt.detector_forward(plan, det, batch, mag)
    vals2, gmag = rt.detector_backward(plan, det, batch, mag, gv)
    torch.cuda.synchronize()
    lo, hi = band
    nb = hi - lo + 1
    T = batch.frames[0]
    D = _oracle_detector(O)
    full = torch.zeros((4, 513, T), dtype=torch.float64)
    full[:, lo:hi + 1, :] = mag.cpu()[:, :nb].double().view(4, T, nb).permute(0, 2, 1)
    full.requires_grad_(True)
    pred = D.forward(full)
    (pred * gv.cpu().double()).sum().backward()
    ref_g = full.grad[:, lo:hi + 1, :].permute(0, 2, 1).reshape(4 * T, nb)
    assert float((vals.cpu().double() - pred.detach()).abs().max()) < 1e-4, band
    assert float((vals2.cpu().double() - pred.detach()).abs().max()) < 1e-4, band
    g = gmag.cpu().double()
    for b in range(4):
        gb, rb = g[b * T:(b + 1) * T, :nb], ref_g[b * T:(b + 1) * T]
        rel = float((gb - rb).norm() / rb.norm())
        assert rel < 1e-4, (band, b, rel)
    assert float(g[:, nb:].abs().max()) == 0.0


_ORC = {}


def _oracle_first(O, band, key, audio, wm_row):
    """fp64 autograd of the first loop body on `band` (the oracle's band indices replaced) + the relative kink distance."""
    if (band, key) in _ORC:
        return _ORC[(band, key)]
    e64 = O.Embedder(dtype=torch.float64)
    e64.band, e64.nonband = O.band_indices(bands=(band[0] * 15.625, band[1] * 15.625))
    assert e64.band[0] == band[0] and e64.band[-1] == band[1]
    a = torch.from_numpy(audio)[None].double()
    m64, p64 = e64.analyse(a)
    c0 = m64[:, e64.band].clone().requires_grad_(True)
    l, p = e64.forward_loss(c0, m64, p64, torch.from_numpy(wm_row).double()[None])
    l.sum().backward()
    kink = float("inf")
    with torch.no_grad():
        mag2, _ = e64.recompute_magnitude(m64, p64)
        mag2[:, e64.nonband] = 0.0
        det = e64.det
        x = det.instance_norm(torch.matmul(det.mel, mag2))
        x = (x - x.mean(dim=(1, 2), keepdim=True)) / (x.std(dim=(1, 2), keepdim=True) + 1e-8)
        x = torch.nn.functional.avg_pool1d(x, 2, 2)
        for w, b in zip(det.ws, det.bs):
            u = det.instance_norm(torch.matmul(w, x) + b[:, None])
            if float(u.abs().max()) > 0:
                kink = min(kink, float(u.abs().min() / u.abs().max()))
            x = torch.nn.functional.leaky_relu(u, 0.2)
    r = dict(loss=float(l.detach()), grad=c0.grad[0].T.contiguous(), kink=kink)      # grad [T, nb]
    _ORC[(band, key)] = r
    return r


def _check_first(rt, O, band, lengths, seed0, combos, nchk):
    plan, det = _plan(rt, band), _det(rt, O, band)
    clips = [make_clip(seed0 + i, n) for i, n in enumerate(lengths)]
    wm = np.stack([(2 * b - 1).astype(np.float32) for _, b in clips])
    batch = rt.Batch(lengths)
    audio = batch.pack([c for c, _ in clips])
    lo, hi = band
    nb = hi - lo + 1
    chk = sorted(set(np.linspace(0, len(lengths) - 1, nchk).astype(int).tolist()))
    first = None
    for pipe, dsp, mel in combos:
        sess = rt.EmbedSession(plan, det, batch, use_graph=False, conv_pipe=pipe, dsp_path=dsp, mel=mel)
        sess.begin(audio, torch.from_numpy(wm).cuda())
        g = sess.gradient()
        torch.cuda.synchronize()
        g, loss = g.cpu().double(), sess.loss.cpu().numpy().copy()
        assert torch.isfinite(g).all()
        assert float(g[:, nb:].abs().max()) == 0.0
        if first is None:
            first = g
        else:
            # all kernel paths agree with each other (rounding level)
            assert float((g - first).norm() / first.norm()) < 2e-3, (band, pipe, dsp, mel)
        for i in chk:
            o = _oracle_first(O, band, (seed0, i, lengths[i]), clips[i][0], wm[i])
            r0, r1 = batch.frame_offsets[i], batch.frame_offsets[i + 1]
            gi, ri = g[r0:r1, :nb], o["grad"]
            assert abs(float(loss[i]) - o["loss"]) < 5e-5 * max(1.0, abs(o["loss"])), (band, i, pipe, dsp, mel)
            rel = float((gi - ri).norm() / ri.norm())
            bar = 5e-4 if o["kink"] > KINK_REL else 2e-2
            assert rel < bar, (band, i, pipe, dsp, mel, rel, o["kink"])
            # the two real bins on their own, relative to their own column (the mel bank gives them little weight, so the
            # band-wide norm would hide a wrong factor in their adjoint: 1/1024 and no imaginary part instead of 1/512)
            for k in (0, 512):
                if lo <= k <= hi:
                    col, rc = gi[:, k - lo], ri[:, k - lo]
                    crel = float((col - rc).norm() / rc.norm())
                    assert crel < (1e-2 if o["kink"] > KINK_REL else 5e-2), (band, k, pipe, dsp, mel, crel)


ALL_COMBOS = [(p, d, m) for p in ("f16x2", "bf16x3", "f32") for d in ("stream", "staged") for m in ("taps", "dense")]


@pytest.mark.parametrize("band", BANDS)
def test_first_gradient_uniform(rt, O, band):
    """32 uniform 1 s clips: loss and dL/dcoef of the first loop body against float64 autograd, per clip (kink rule of
    tests/test_gpu_conv_scales.py), under every conv pipe, both DSP paths and both mel settings."""
    _check_first(rt, O, band, [16000] * 32, 300, ALL_COMBOS, 4)


@pytest.mark.parametrize("band", BANDS)
def test_first_gradient_ragged(rt, O, band):
    """A ragged 1-10 s batch (ragged GEMMs, three-kernel read-out) on both DSP paths."""
    lengths = [16000, 160000, 48000, 23456, 100001, 64000, 32000, 128000]
    _check_first(rt, O, band, lengths, 400, [("f16x2", "stream", "taps"), ("f32", "staged", "dense")], 3)


@pytest.mark.parametrize("band", [(0, 512), (20, 448)])
def test_silent_and_tiny_clips_finite(rt, O, band):
    """A silent clip and a clip scaled by 1e-30 inside a 32-clip batch: every output of 8 iterations is finite."""
    lengths = [16000] * 32
    clips = [make_clip(500 + i, 16000)[0] for i in range(32)]
    clips[3] = np.zeros(16000, np.float32)
    clips[17] = (clips[17] * 1e-30).astype(np.float32)
    wm = np.stack([(2 * make_clip(500 + i, 16000)[1] - 1).astype(np.float32) for i in range(32)])
    plan, det = _plan(rt, band), _det(rt, O, band)
    batch = rt.Batch(lengths)
    sess = rt.EmbedSession(plan, det, batch, num_iterations=8, use_graph=True)
    sess.begin(batch.pack(clips), torch.from_numpy(wm).cuda())
    sess.iterate(8)
    out = sess.finish()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert torch.isfinite(sess.loss).all() and torch.isfinite(sess.best_loss).all()
    assert torch.isfinite(sess.best_coef).all()


@pytest.mark.parametrize("hz", [(0, 8000), (300, 7000)])
def test_edited_card_service_roundtrip(hz):
    """load() of a card whose embedding_bands is edited, then embed_watermark / detect_watermark, mono and stereo: BER 0."""
    import yaml
    from aware_amd.utils.models import load
    from aware_amd.utils.models import load_model
    from aware_amd.service.embed import embed_watermark
    from aware_amd.service.detect import detect_watermark
    with open(load_model._CARD) as f:
        card = yaml.safe_load(f)
    card["embedding_bands"] = list(hz)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "card.yaml")
        with open(p, "w") as f:
            yaml.safe_dump(card, f)
        embedder, detector = load(p)
    assert embedder._plan(16000).band_stride == 576
    rng = np.random.default_rng(11)
    bits = rng.integers(0, 2, 20).astype(np.int32)
    mono = (0.1 * rng.standard_normal(32000)).astype(np.float32)
    out = embed_watermark(mono, 16000, bits, embedder)
    got = np.asarray(detect_watermark(out, 16000, detector)).reshape(-1)[:20]
    assert np.array_equal(got.astype(np.int32), bits), (hz, got, bits)
    stereo = (0.1 * rng.standard_normal((32000, 2))).astype(np.float32)
    out2 = embed_watermark(stereo, 16000, bits, embedder)
    got2 = detect_watermark(out2, 16000, detector)
    for ch in (got2 if isinstance(got2, (list, tuple)) else [got2]):
        assert np.array_equal(np.asarray(ch).reshape(-1)[:20].astype(np.int32), bits), (hz, ch, bits)


def test_training_extension_refuses_wide_band(rt, O):
    """The detector-training extension serves the narrow layout only: AWARE_E_UNSUPPORTED from the C ABI, NotImplementedError
    from the wrappers."""
    import ctypes as C
    band = (20, 448)
    plan, det = _plan(rt, band), _det(rt, O, band)
    batch = rt.Batch([16000] * 2)
    mag, _ = rt.stft_band(plan, batch, batch.pack([make_clip(1, 16000)[0], make_clip(2, 16000)[0]]))
    with pytest.raises(NotImplementedError):
        rt.detector_weight_gradients(plan, det, batch, mag, torch.ones((2, 20), device="cuda"))
    with pytest.raises(NotImplementedError):
        rt.detector_train_gradients(plan, det, batch, mag, torch.ones((2, 20), device="cuda"))
    lib = plan.lib
    nbytes = lib.aware_detector_train_workspace_bytes(batch.h, det.h)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    gm = torch.empty((batch.total_frames, plan.band_stride), device="cuda")
    gw = [torch.empty((det.channels[i + 1], det.channels[i]), device="cuda") for i in range(len(det.channels) - 1)]
    pw = (C.c_void_p * len(gw))(*[t.data_ptr() for t in gw])
    gv = torch.ones((2, 20), device="cuda")
    rc = lib.aware_detector_weight_gradients(det.h, batch.h, C.c_void_p(mag.data_ptr()), C.c_void_p(gv.data_ptr()), None,
                                             C.c_void_p(gm.data_ptr()), pw, None, C.c_void_p(ws.data_ptr()), nbytes, None)
    assert rc == -2


@pytest.mark.parametrize("band", [(0, 512), (256, 512)])
def test_staged_and_streaming_analysis_agree(rt, O, band):
    """The analysis of aware_embed_begin on both DSP paths (streaming wide form; staged kernel with its Nyquist slot and tail
    loop) against aware_stft_band: band magnitudes and phasors of the original clips, zero tail."""
    lengths = [16000, 48000, 23456]
    clips = [make_clip(90 + i, n) for i, n in enumerate(lengths)]
    wm = torch.from_numpy(np.stack([(2 * b - 1).astype(np.float32) for _, b in clips])).cuda()
    plan, det = _plan(rt, band), _det(rt, O, band)
    batch = rt.Batch(lengths)
    audio = batch.pack([c for c, _ in clips])
    mag, ph = rt.stft_band(plan, batch, audio, normalize=True)
    S = plan.band_stride
    nb = band[1] - band[0] + 1
    for dsp in ("stream", "staged"):
        sess = rt.EmbedSession(plan, det, batch, use_graph=False, dsp_path=dsp)
        sess.begin(audio, wm)
        torch.cuda.synchronize()
        m = sess._view(10, (batch.total_frames, S)).cpu()
        p = sess._view(7, (batch.total_frames, S), torch.complex64).cpu()
        ref = mag.cpu()
        assert float((m - ref).abs().max()) <= 1e-5 * float(ref.abs().max()), dsp
        assert float(m[:, nb:].abs().max()) == 0.0
        sig = ref[:, :nb] > 1e-3 * ref.max()
        assert float((p[:, :nb] - ph.cpu()[:, :nb]).abs()[sig].max()) < 1e-4, dsp


@pytest.mark.parametrize("band", [(0, 512), (20, 448)])
def test_push_extremes_l1_first_gradient(rt, O, band):
    """The loss push_extremes + L1 at a band of the wide layout (the L1 sum in the wide synthesis, its sign term in the wide
    analysis adjoint): loss and dL/dcoef of the first loop body after 3 steps have moved the coefficients off c0, against
    float64 autograd of the oracle's loss on the session's own coefficients."""
    w = 0.5
    plan, det = _plan(rt, band), _det(rt, O, band)
    lengths = [16000] * 4
    clips = [make_clip(700 + i, n) for i, n in enumerate(lengths)]
    wm = np.stack([(2 * b - 1).astype(np.float32) for _, b in clips])
    batch = rt.Batch(lengths)
    sess = rt.EmbedSession(plan, det, batch, num_iterations=8, use_graph=False, loss="push_extremes_l1", l1_weight=w)
    sess.begin(batch.pack([c for c, _ in clips]), torch.from_numpy(wm).cuda())
    sess.iterate(3)
    coef = sess.coef.cpu().double().clone()
    g = sess.gradient().cpu().double()
    loss = sess.loss.cpu().numpy().copy()
    lo, hi = band
    nb = hi - lo + 1
    assert float(g[:, nb:].abs().max()) == 0.0
    for i in range(4):
        e64 = O.Embedder(dtype=torch.float64, loss="push_extremes_l1", l1_weight=w)
        e64.band, e64.nonband = O.band_indices(bands=(lo * 15.625, hi * 15.625))
        a = torch.from_numpy(clips[i][0])[None].double()
        m64, p64 = e64.analyse(a)
        r0, r1 = batch.frame_offsets[i], batch.frame_offsets[i + 1]
        c = coef[r0:r1, :nb].T[None].clone().requires_grad_(True)        # [1, nb, T]
        assert float((c.detach() - m64[:, e64.band]).abs().max()) > 0   # the L1 term is away from its kink at c0
        l, _ = e64.forward_loss(c, m64, p64, torch.from_numpy(wm[i]).double()[None])
        l.sum().backward()
        ref = c.grad[0].T
        assert abs(float(loss[i]) - float(l)) < 5e-5, (band, i, float(loss[i]), float(l))
        rel = float((g[r0:r1, :nb] - ref).norm() / ref.norm())
        assert rel < 5e-4, (band, i, rel)
        for k in (0, 512):
            if lo <= k <= hi:
                crel = float((g[r0:r1, k - lo] - ref[:, k - lo]).norm() / ref[:, k - lo].norm())
                assert crel < 1e-2, (band, i, k, crel)


@pytest.mark.parametrize("band", [(0, 512), (64, 384)])
@pytest.mark.parametrize("dsp", ["stream", "staged"])
def test_fused_nadam_steps_over_the_wide_row(rt, O, band, dsp):
    """Six iterations of the fused loop (NAdam + clamp + best snapshot over the wide row, in the epilogue of the streaming or
    the staged analysis adjoint), each against a float64 host restatement of the step (torch.optim.NAdam + clamp to the box,
    multibit_embedder.py:112-122) applied to the gradient the session reports at the same point (aware_embed_gradient, which
    changes no state); the losses against the oracle's loop.  (Coefficients are compared step by step rather than against an
    independent trajectory: a push_extremes / LeakyReLU kink flip between two f32 implementations moves whole frames apart
    after a few steps, on the model card's band as much as on a wide one.)"""
    n = 6
    plan, det = _plan(rt, band), _det(rt, O, band)
    lengths = [16000, 16000, 48000]
    clips = [make_clip(800 + i, l) for i, l in enumerate(lengths)]
    wm = np.stack([(2 * b - 1).astype(np.float32) for _, b in clips])
    batch = rt.Batch(lengths)
    sess = rt.EmbedSession(plan, det, batch, num_iterations=n, use_graph=False, dsp_path=dsp)
    sess.begin(batch.pack([c for c, _ in clips]), torch.from_numpy(wm).cuda())
    nb = band[1] - band[0] + 1
    cg, cm, bc2 = O.nadam_schedule(n)
    c0 = sess.coef.cpu().double().clone()
    lo, hi = c0 * (1 - 10 ** (-6.0 / 20)), c0 * (1 + 10 ** (-6.0 / 20))
    lo = lo.clamp_min(0)
    p = c0.clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    best_loss = np.full(len(lengths), np.inf)
    best = c0.clone()
    fo = batch.frame_offsets
    traj = []
    for it in range(n):
        g = sess.gradient().cpu().double()
        loss = sess.loss.cpu().numpy().copy()
        traj.append(loss)
        sess.iterate(1)
        got = sess.coef.cpu().double()
        O.nadam_step(p, g, m, v, cg[it], cm[it], bc2[it])
        p = torch.minimum(torch.maximum(p, lo), hi)
        err = (got - p).abs() / (1e-3 + p.abs())
        assert float(err[:, :nb].max()) < 2e-4, (band, dsp, it, float(err.max()))
        assert float(got[:, nb:].abs().max()) == 0.0
        for i in range(len(lengths)):
            if loss[i] < best_loss[i]:
                best_loss[i] = loss[i]
                best[fo[i]:fo[i + 1]] = got[fo[i]:fo[i + 1]]
        np.testing.assert_array_equal(sess.best_coef.cpu().double().numpy(), best.numpy())
        p = got.clone()            # the next step starts where the kernel left off (moments carried on the host)
    traj = np.stack(traj)
    # the per-step losses against the oracle's own loop (f32), per clip
    for i in range(len(lengths)):
        ref = []
        emb = O.Embedder(num_iterations=n)
        emb.band, emb.nonband = O.band_indices(bands=(band[0] * 15.625, band[1] * 15.625))
        emb.embed(clips[i][0][None], wm[i][None], record=lambda it, l, pr, g: ref.append(float(l[0])))
        assert np.max(np.abs(np.asarray(ref) - traj[:, i])) < 1e-3, (band, dsp, i, ref, traj[:, i])


@pytest.mark.parametrize("band_hz", [(0, 8000), (1000, 6000)])
def test_registry_optimizer_steps_vs_oracle(rt, band_hz):
    """An optimiser of the registry (Adam with a cosine schedule: the separate opt_rows step over the wide row) against the
    oracle's torch.optim loop on one clip, per-step losses."""
    from aware_amd.embedding import AWAREEmbedder
    from oracle import aware_oracle as O
    n = 6
    emb = AWAREEmbedder(embedding_bands=band_hz, num_iterations=n, verbose=False, use_graph=False, loss="push_extremes",
                        optimizer_cfg={"name": "adam", "params": {"lr": 0.05}},
                        scheduler_cfg={"name": "cosine_annealing", "params": {"T_max": n}})
    audio, bits = make_clip(3, 16000)
    wm = O.bits_to_bipolar(bits).astype(np.float32)
    batch = rt.Batch([16000])
    sess = emb.start_session(batch, 16000)
    assert sess.plan.band_stride == 576
    sess.begin(batch.pack([audio]), torch.from_numpy(wm)[None].cuda())
    mine = []
    for _ in range(n):
        sess.iterate(1)
        mine.append(float(sess.loss.cpu()[0]))
    lo, hi = sess.plan.band_bins
    ref = []
    oe = O.Embedder(num_iterations=n, optimizer="adam", optimizer_params={"lr": 0.05}, scheduler="cosine_annealing",
                    scheduler_params={"T_max": n})
    oe.band, oe.nonband = O.band_indices(bands=(lo * 15.625, hi * 15.625))
    oe.embed_registry(audio[None], wm[None], record=lambda it, l, lr: ref.append(l))
    d = np.abs(np.asarray(mine) - np.asarray(ref))
    assert d.max() < 1e-3, (band_hz, mine, ref)


@pytest.mark.parametrize("band", [(0, 512), (20, 448)])
@pytest.mark.parametrize("key", ["gelu_instance_tanh", "relu_none_sigmoid"])
def test_variant_detector_wide_band_vs_float64(rt, band, key):
    """aware_detector_forward / _backward of an architecture variant (staged route, melT / melB at stride 576) against the
    float64 restatement of the variant: values to 5e-5, magnitude gradient per clip to 1e-4 relative L2 (kink-checked)."""
    from aware_amd.detection import AWAREDetectorNet
    from test_detector_variants_host import VariantDetector, push_extremes_sum, split_key
    act, norm, fin = split_key(key)
    net = AWAREDetectorNet(activation=act, norm_layer=norm, final_activation=fin)
    plan = _plan(rt, band)
    dev = net.device_weights(plan)
    assert not dev.is_card
    lengths = [16000] * 6 + [48000, 23456]
    batch = rt.Batch(lengths)
    lo, hi = band
    nb = hi - lo + 1
    rng = np.random.default_rng(sum(band))
    mags = []
    rows = torch.zeros((batch.total_frames, plan.band_stride), dtype=torch.float32)
    for i, T in enumerate(batch.frames):
        m = np.zeros((513, T), np.float32)
        z = rng.standard_normal((nb, T, 2))
        m[lo:hi + 1] = 0.3 * np.hypot(z[..., 0], z[..., 1])
        mags.append(m)
        rows[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :nb] = torch.from_numpy(m[lo:hi + 1].T)
    rows = rows.cuda()
    target = torch.from_numpy(np.where(rng.integers(0, 2, (batch.B, 20)) > 0, 1.0, -1.0).astype(np.float32))
    vals = rt.detector_forward(plan, dev, batch, rows)
    p = vals.detach().clone().requires_grad_(True)
    push_extremes_sum(p, target.cuda()).backward()
    vals2, gmag = rt.detector_backward(plan, dev, batch, rows, p.grad)
    vals, vals2, gmag = vals.cpu().numpy(), vals2.cpu().numpy(), gmag.cpu().numpy()
    np.testing.assert_array_equal(vals, vals2)
    assert np.max(np.abs(gmag[:, nb:])) == 0.0
    vd = VariantDetector(net)
    for i, m in enumerate(mags):
        x = torch.from_numpy(m).double()[None].requires_grad_(True)
        ref = vd.forward(x)
        push_extremes_sum(ref, target[i:i + 1].double()).backward()
        np.testing.assert_allclose(vals[i], ref.detach().numpy()[0], atol=5e-5)
        mine = gmag[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :nb].T
        r = x.grad.numpy()[0, lo:hi + 1]
        rel = float(np.linalg.norm(mine - r) / np.linalg.norm(r))
        kink = vd.kink_distance(x.detach())[0]
        assert rel < (1e-4 if kink > 1e-5 else 2e-2), (band, key, i, rel, kink)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide_band.npz")
GOLDEN_BANDS = {"0_8000": ((0, 8000), (0, 512)), "300_7000": ((300, 7000), (20, 448))}


@pytest.mark.parametrize("band", list(GOLDEN_BANDS))
def test_detector_seam_vs_reference(rt, band):
    """AWAREDetectorNet.forward (plug-in seam) of an embedder's net at a wide band against the reference's predictions and
    in-band magnitude gradients (tests/golden/wide_band.npz, tools/make_golden_wide_band.py)."""
    from aware_amd.embedding import AWAREEmbedder
    from test_detector_variants_host import push_extremes_sum
    from test_wide_band_host import golden_magnitudes
    fx = np.load(GOLDEN)
    hz, (lo, hi) = GOLDEN_BANDS[band]
    net = AWAREEmbedder(embedding_bands=hz, verbose=False, loss="push_extremes").detection_net
    assert net.band_plan().band_bins == (lo, hi)
    mag = torch.from_numpy(golden_magnitudes(lo, hi)).cuda().requires_grad_(True)
    pred = net.forward(mag)
    np.testing.assert_allclose(pred.detach().cpu().numpy(), fx[f"net/{band}/pred"], atol=5e-5)
    push_extremes_sum(pred, torch.from_numpy(fx["target"]).cuda()).backward()
    g = mag.grad.cpu().numpy()[:, lo:hi + 1, ::int(fx["grad_step"])]
    assert np.max(np.abs(mag.grad.cpu().numpy()[:, ~_mask((lo, hi))]), initial=0.0) == 0.0
    for b in range(2):
        r = fx[f"net/{band}/grad"][b]
        assert np.linalg.norm(g[b] - r) / np.linalg.norm(r) < 2e-4, (band, b)


@pytest.mark.parametrize("band", list(GOLDEN_BANDS))
def test_embed_trajectory_400_steps_vs_reference(rt, band):
    """The reference's own 400-step embed of the 1 s seed clip with the card's embedding_bands edited: every step's loss
    within 1.6e-2, the watermarked waveform within 0.15 relative L2, the detected bits equal."""
    from aware_amd.embedding import AWAREEmbedder
    from oracle import aware_oracle as O
    fx = np.load(GOLDEN)
    hz, bins = GOLDEN_BANDS[band]
    emb = AWAREEmbedder(embedding_bands=hz, verbose=False, loss="push_extremes")
    audio, bits = make_clip(1, 16000)
    wm = O.bits_to_bipolar(bits).astype(np.float32)[None]
    batch = rt.Batch([16000])
    sess = emb.start_session(batch, 16000)
    assert sess.plan.band_bins == bins
    sess.begin(batch.pack([audio]), torch.from_numpy(wm).cuda())
    mine = []
    for _ in range(400):
        sess.iterate(1)
        mine.append(float(sess.loss.cpu()[0]))
    d = np.abs(np.asarray(mine) - fx[f"traj/{band}/losses"])
    print(f"{band}: |loss - reference| step0 {d[0]:.2e} max {d.max():.2e}")
    assert d[0] < 1e-5 and d.max() <= 1.6e-2
    out = sess.finish(torch.tensor([float(np.max(audio))], device="cuda"))
    out_c = out.cpu().numpy()
    assert out_c.shape[0] == int(fx[f"traj/{band}/out_len"])
    r = fx[f"traj/{band}/out_sample"]
    rel = np.linalg.norm(out_c[::int(fx[f"traj/{band}/out_step"])] - r) / np.linalg.norm(r)
    print(f"{band}: waveform rel L2 to the reference {rel:.3e}")
    assert rel <= 0.15
    plan = sess.plan
    vals = rt.detect(plan, emb.detection_net.device_weights(plan), rt.Batch([out_c.shape[0]]), out).cpu().numpy()[0]
    np.testing.assert_array_equal(O.decode_bits(vals), fx[f"traj/{band}/det_bits"])


@pytest.mark.parametrize("band_hz", [(0, 8000), (300, 7000)])
def test_reference_shaped_loop_matches_fused_loop(rt, band_hz):
    """Five iterations of AWAREEmbedder._optimize as the reference writes it (plug-in lists, the net under autograd through the
    seam, loss.backward(), NAdam + clamp) against the fused session on the same clip, at a band of the wide layout."""
    from aware_amd.embedding import AWAREEmbedder
    from aware_amd.embedding.losses import get_loss_fn
    from oracle import aware_oracle as O
    emb = AWAREEmbedder(embedding_bands=band_hz, loss="push_extremes", verbose=False)
    audio, bits = make_clip(1, 16000)
    target = torch.from_numpy(O.bits_to_bipolar(bits).astype(np.float32)).cuda()
    pre, post = emb.audio_preprocess_pipeline, emb.audio_postprocess_pipeline
    v = torch.from_numpy(audio).cuda()
    for p in pre:
        v = p(v)
    magnitude, phase = v
    fi, nfi = emb._get_embedding_frequency_indices(16000, 1024)
    nb = len(fi)
    fi_t, nfi_t = torch.from_numpy(fi).cuda(), torch.from_numpy(nfi).cuda()
    c0 = magnitude[fi_t].flatten().detach().clone()
    delta = c0 * 10 ** (-emb.tolerance_db / 20)
    lo, hi = torch.clamp(c0 - delta, min=0), c0 + delta
    coeffs = c0.clone().requires_grad_(True)
    opt = rt.NAdamClamp(coeffs.data, lr=0.1)
    loss_fn = get_loss_fn("push_extremes")
    losses, grad1 = [], None
    for it in range(5):
        coeffs.grad = None
        wmag = magnitude.detach().clone()
        wmag[fi_t] = coeffs.reshape(nb, -1)
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
    batch = rt.Batch([16000])
    sess = emb.start_session(batch, 16000)
    sess.begin(batch.pack([audio]), target[None])
    gf = sess.gradient()[:, :nb].T.flatten()
    fused = []
    for it in range(5):
        sess.iterate(1)
        fused.append(float(sess.loss.cpu()[0]))
    assert abs(losses[0] - fused[0]) < 5e-6, (losses[0], fused[0])
    rel = float((grad1 - gf).norm() / gf.norm())
    print(band_hz, "first gradient, plug-in seam vs fused loop, rel L2:", rel, "| losses", losses, fused)
    assert rel < 5e-5, rel
    assert np.max(np.abs(np.asarray(losses) - np.asarray(fused))) < 1e-3
    cf = sess.coef[:, :nb].T.flatten()
    frac = float(((coeffs.detach() - cf).abs() <= 1e-3 * (1 + cf.abs())).float().mean())
    assert frac > 0.995, frac
