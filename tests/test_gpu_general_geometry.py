"""The embed / detect loop on the general route (key general_geometry) on the device, against the
geometry-generic restatement of tests/test_general_geometry_host.py (GeneralLoop) and, at the card geometry, against the
card route itself.

Geometries: G1 256 / 64 / 256 hann; G2 512 / 200 / 400 hamming (the hop does not divide n_fft; NOLA holds, checked below);
G3 the card's 1024 / 256 / 1024 with the key on; G4 2048 / 512 / 2048 at 44.1 kHz (a 162-bin band out of 1025); G5 4096 /
1024 / 4096 with the band [0, 8000] Hz: all 2049 bins, rows of 2112 floats.  Batches are ragged: the shortest clip the
geometry takes (n_fft/2 + 1 samples), one with an odd and one with an even frame count, one of about a second.

The shortest clip has two or three frames, so one pooled frame: every block's InstanceNorm reads 0, the values are
tanh(0) = 0, the loss is 1 and the gradient 0 whatever the spectrum holds.  Its synthesis is n_fft/2 samples or fewer, which
torch.stft refuses to pad, so for the loop the restatement is not run on it and those figures are asserted instead (as
tests/test_gpu_long_clips.py does for the card route's 513-sample clip).

Run on the MI355X box:  python -m pytest tests/test_gpu_general_geometry.py -m gpu -q -s
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import make_clip
from test_general_geometry_host import GeneralLoop

pytestmark = pytest.mark.gpu

# name: n_fft, hop, win_length, window, sample rate, band (Hz), about one second
GEOM = {
    "G1": (256, 64, 256, "hann", 16000, (500, 4000), 16000),
    "G2": (512, 200, 400, "hamming", 16000, (500, 4000), 16000),
    "G3": (1024, 256, 1024, "hann", 16000, (500, 4000), 16000),
    "G4": (2048, 512, 2048, "hann", 44100, (500, 4000), 44100),
    "G5": (4096, 1024, 4096, "hann", 16000, (0, 8000), 16000),
}
STRIDE = {"G1": 64, "G2": 128, "G3": 256, "G4": 192, "G5": 2112}
SENTINEL = -7.5


def lengths_of(name):
    """The ragged batch of a geometry: the second-long clip first, then odd T, the shortest clip, even T."""
    n_fft, hop, *_, second = GEOM[name]
    odd = hop * 10 + 3                 # T = 11
    even = hop * 13 + hop // 2         # T = 14
    assert odd > n_fft // 2 and (1 + odd // hop) % 2 == 1 and (1 + even // hop) % 2 == 0
    return [second, odd, n_fft // 2 + 1, even]


@pytest.fixture(scope="module")
def rt():
    from aware_amd import runtime
    from aware_amd._lib import require_gpu
    require_gpu()
    return runtime


_CASES = {}


def case(rt, name):
    """Embedder, detector, plan, device detector, batch, clips, payloads of a geometry: built once, shared, never modified."""
    if name not in _CASES:
        from aware_amd.detection import AWAREDetector
        from aware_amd.embedding import AWAREEmbedder
        n_fft, hop, win, window, sr, band, _ = GEOM[name]
        emb = AWAREEmbedder(frame_length=n_fft, hop_length=hop, win_length=win, window=window, embedding_bands=band,
                            general_geometry=True, verbose=False, loss="push_extremes", use_graph=False,
                            detection_net_cfg={"n_fft": n_fft, "sample_rate": sr})
        det = AWAREDetector(emb.detection_net, frame_length=n_fft, hop_length=hop, win_length=win, window=window,
                            embedding_bands=band, general_geometry=True)
        lengths = lengths_of(name)
        assert all(rt.nola_ok(n_fft, hop, win, window, n) for n in lengths)
        clips = [make_clip(300 + i, n) for i, n in enumerate(lengths)]
        wm = np.stack([(2 * b - 1).astype(np.float32) for _, b in clips])
        plan = emb._plan(sr)
        assert plan.general and plan.band_stride == STRIDE[name] and plan.spectrum_stride >= n_fft // 2 + 1
        batch = emb.make_batch(lengths, sr)
        assert batch.frames == [1 + n // hop for n in lengths]
        assert batch.out_lengths == [hop * (t - 1) for t in batch.frames]
        assert batch.total_pooled >= sum(t // 2 for t in batch.frames)
        _CASES[name] = dict(emb=emb, det=det, plan=plan, dev=emb.detection_net.device_weights(plan), batch=batch,
                            clips=[c for c, _ in clips], wm=wm, sr=sr, lengths=lengths)
    return _CASES[name]


_REFS = {}


def loop64(name, **kw):
    n_fft, hop, win, window, sr, band, _ = GEOM[name]
    return GeneralLoop(n_fft, hop, win, window, sr, band, dtype=torch.float64, **kw)


def loop32(name, **kw):
    n_fft, hop, win, window, sr, band, _ = GEOM[name]
    return GeneralLoop(n_fft, hop, win, window, sr, band, **kw)


def trivial(name, i):
    """The clip has one pooled frame and a synthesis torch.stft cannot pad: values 0, loss 1, gradient 0 (module docstring)."""
    n_fft, hop, *_ = GEOM[name]
    n = lengths_of(name)[i]
    return (1 + n // hop) // 2 == 1 and hop * (n // hop) <= n_fft // 2


def reference(rt, name):
    """float64 restatement per clip: detect values, and loss / gradient [T, nband] of the first loop body."""
    if name not in _REFS:
        c = case(rt, name)
        e64 = loop64(name)
        out = []
        for i, (clip, wm) in enumerate(zip(c["clips"], c["wm"])):
            vals = e64.detect_raw(torch.from_numpy(clip).double()[None])[0].numpy()
            if trivial(name, i):
                out.append(dict(vals=vals, loss=1.0, grad=None))
            else:
                loss, _, g = e64.first_iteration(torch.from_numpy(clip).double()[None], torch.from_numpy(wm).double()[None])
                out.append(dict(vals=vals, loss=float(loss[0]), grad=g[0].T.contiguous()))
        _REFS[name] = out
    return _REFS[name]


def test_g2_passes_nola_on_the_host(rt):
    n_fft, hop, win, window, *_ = GEOM["G2"]
    assert n_fft % hop != 0 and all(rt.nola_ok(n_fft, hop, win, window, n) for n in lengths_of("G2"))


@pytest.mark.parametrize("name", list(GEOM))
def test_detect(rt, name):
    """aware_detect on the general route (gen_stft -> band_mag -> det_forward -> read-out) against the float64 restatement:
    1e-4, the bound of tests/test_gpu_wide_band.py for the same values; through detect_batch and detect_device."""
    c = case(rt, name)
    ref = reference(rt, name)
    vals = c["det"].detect_batch(c["clips"], c["sr"]).cpu().numpy()
    vals2 = c["det"].detect_device(c["batch"].pack(c["clips"]), c["batch"], c["sr"]).cpu().numpy()
    err = [float(np.max(np.abs(vals[i] - r["vals"]))) for i, r in enumerate(ref)]
    print(f"{name}: max |detect - float64 restatement| per clip {['%.1e' % e for e in err]} (bound 1e-4)")
    assert np.isfinite(vals).all() and np.array_equal(vals, vals2)
    assert max(err) < 1e-4, (name, err)
    short = lengths_of(name).index(GEOM[name][0] // 2 + 1)
    assert float(np.abs(vals[short]).max()) == 0.0          # one pooled frame


@pytest.mark.parametrize("pipe", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("name", list(GEOM))
def test_first_step(rt, name, pipe):
    """Loss and aware_embed_gradient of the first loop body against the float64 restatement's autograd, on both conv pipes:
    loss 5e-5 * max(1, |loss|), gradient relative L2 2e-4 on bf16x3 and 2e-3 on f16x2 (the bounds of
    tests/test_gpu_wide_band.py).  Padding columns of the gradient rows stay zero."""
    c = case(rt, name)
    ref = reference(rt, name)
    batch, plan = c["batch"], c["plan"]
    sess = rt.EmbedSession(plan, c["dev"], batch, use_graph=False, conv_pipe=pipe)
    sess.begin(batch.pack(c["clips"]), torch.from_numpy(c["wm"]).cuda())
    g = sess.gradient()
    torch.cuda.synchronize()
    g, loss = g.cpu().double(), sess.loss.cpu().numpy().copy()
    nb = plan.nband
    assert torch.isfinite(g).all() and np.isfinite(loss).all()
    assert g.shape[1] == STRIDE[name] and (nb == g.shape[1] or float(g[:, nb:].abs().max()) == 0.0)
    bar = {"bf16x3": 2e-4, "f16x2": 2e-3}[pipe]
    figures = []
    for i, r in enumerate(ref):
        r0, r1 = batch.frame_offsets[i], batch.frame_offsets[i + 1]
        el = abs(float(loss[i]) - r["loss"]) / max(1.0, abs(r["loss"]))
        rel = float(g[r0:r1].abs().max()) if r["grad"] is None else float((g[r0:r1, :nb] - r["grad"]).norm() / r["grad"].norm())
        figures.append((i, el, rel, r["grad"] is None))
        print(f"{name} {pipe} clip {i} (n = {c['lengths'][i]}): loss err {el:.1e} (bound 5e-5), gradient "
              f"{'max |g| %.1e (must be 0)' % rel if r['grad'] is None else 'rel L2 %.2e (bound %.0e)' % (rel, bar)}")
    for i, el, rel, zero in figures:
        assert el < 5e-5, (name, pipe, i, el)
        assert rel == 0.0 if zero else rel < bar, (name, pipe, i, rel)


@pytest.mark.parametrize("name", list(GEOM))
def test_trajectory(rt, name):
    """Five steps of the loop (assemble, synthesis, two normalisers, analysis, band_mag, detector, their backward, the fused
    NAdam step): per-step losses within 1e-3 of the float32 restatement's own loop, and lo <= coef <= hi after every step."""
    n = 5
    c = case(rt, name)
    batch, plan = c["batch"], c["plan"]
    sess = rt.EmbedSession(plan, c["dev"], batch, num_iterations=n, use_graph=False)
    sess.begin(batch.pack(c["clips"]), torch.from_numpy(c["wm"]).cuda())
    lo, hi = (t.clone() for t in sess.bounds)
    assert bool((lo <= hi).all()) and bool((lo >= 0).all())
    mine = []
    for _ in range(n):
        sess.iterate(1)
        mine.append(sess.loss.cpu().numpy().copy())
        coef = sess.coef
        assert bool((coef >= lo).all()) and bool((coef <= hi).all())
        assert plan.nband == plan.band_stride or float(coef[:, plan.nband:].abs().max()) == 0.0
    mine = np.stack(mine)
    for i, (clip, wm) in enumerate(zip(c["clips"], c["wm"])):
        if trivial(name, i):
            ref = np.ones(n)
        else:
            ref = []
            loop32(name, num_iterations=n).embed(clip[None], wm[None], record=lambda it, l, *_: ref.append(float(l[0])))
        d = np.abs(mine[:, i] - np.asarray(ref))
        print(f"{name} clip {i}: losses {np.round(mine[:, i], 5).tolist()}, max |mine - restatement| {d.max():.1e} (bound 1e-3)")
        assert d.max() < 1e-3, (name, i, mine[:, i], ref)


def test_outputs_stay_between_sentinels(rt):
    """aware_embed_finish writes clip b's hop * (T_b - 1) samples at out_off[b] and nothing else (G2: hop 200, ragged)."""
    c = case(rt, "G2")
    batch = c["batch"]
    sess = rt.EmbedSession(c["plan"], c["dev"], batch, num_iterations=2, use_graph=False)
    sess.begin(batch.pack(c["clips"]), torch.from_numpy(c["wm"]).cuda())
    sess.iterate(2)
    pad = 64
    buf = torch.full((batch.total_out + 2 * pad,), SENTINEL, device="cuda")
    out = buf[pad:pad + batch.total_out]
    rt.check(sess.lib.aware_embed_finish(sess.h, None, C.c_void_p(out.data_ptr()), None), "aware_embed_finish")
    torch.cuda.synchronize()
    assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + batch.total_out:] == SENTINEL).all())
    assert batch.out_offsets == np.concatenate([[0], np.cumsum(batch.out_lengths)[:-1]]).tolist()
    for o, m in zip(batch.out_offsets, batch.out_lengths):
        y = out[o:o + m]
        assert bool(torch.isfinite(y).all()) and abs(float(y.abs().max()) - 1.0) < 1e-6      # normalised once, all written
    vals = torch.full((batch.B + 2, 20), SENTINEL, device="cuda")
    nbytes = sess.lib.aware_detect_workspace_bytes(batch.h, c["dev"].h)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rt.check(sess.lib.aware_detect(c["plan"].h, c["dev"].h, batch.h, C.c_void_p(batch.pack(c["clips"]).data_ptr()),
                                   C.c_void_p(vals[1:].data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, None), "aware_detect")
    torch.cuda.synchronize()
    assert bool((vals[0] == SENTINEL).all()) and bool((vals[-1] == SENTINEL).all()) and bool((vals[1:-1].abs() <= 1).all())


def test_card_geometry_on_both_routes(rt):
    """G3 needs no reference: the general route against the card route on the same clips and payloads.  detect values to
    1e-5, the first gradient to 2e-4 relative L2 on bf16x3, five losses to 1e-3; and the card route's own results are bit for
    bit what they were before any general plan, batch, detector or session existed in the process."""
    from oracle import aware_oracle as O
    lengths = lengths_of("G3")
    clips = [make_clip(300 + i, n)[0] for i, n in enumerate(lengths)]
    wm = np.stack([(2 * make_clip(300 + i, n)[1] - 1).astype(np.float32) for i, n in enumerate(lengths)])
    ws, bs = O.detector_weights()

    def card_run():
        plan = rt.Plan()
        det = rt.DetectorWeights(plan, O.mel_filter_bank(), [w.numpy() for w in ws], [b.numpy() for b in bs])
        batch = rt.Batch(lengths)
        audio = batch.pack(clips)
        vals = rt.detect(plan, det, batch, audio).cpu()
        sess = rt.EmbedSession(plan, det, batch, num_iterations=5, use_graph=False, conv_pipe="bf16x3")
        sess.begin(audio, torch.from_numpy(wm).cuda())
        g = sess.gradient().cpu()
        losses = []
        for _ in range(5):
            sess.iterate(1)
            losses.append(sess.loss.cpu().clone())
        return vals, g, torch.stack(losses), sess.finish().cpu(), batch

    before = card_run()
    plan = rt.Plan(general=True)
    assert plan.general and plan.band_stride == 256 and plan.nband == 225
    det = rt.DetectorWeights(plan, O.mel_filter_bank(), [w.numpy() for w in ws], [b.numpy() for b in bs])
    batch = rt.Batch(lengths, plan=plan)
    audio = batch.pack(clips)
    vals = rt.detect(plan, det, batch, audio).cpu()
    sess = rt.EmbedSession(plan, det, batch, num_iterations=5, use_graph=False, conv_pipe="bf16x3")
    sess.begin(audio, torch.from_numpy(wm).cuda())
    g = sess.gradient().cpu()
    losses = []
    for _ in range(5):
        sess.iterate(1)
        losses.append(sess.loss.cpu().clone())
    losses = torch.stack(losses)
    out = sess.finish().cpu()
    after = card_run()
    for a, b in zip(before[:4], after[:4]):
        assert torch.equal(a, b)
    cb = before[4]
    assert batch.frames == cb.frames and batch.out_offsets == cb.out_offsets and batch.out_lengths == cb.out_lengths
    dv = float((vals - before[0]).abs().max())
    rel = []
    for i in range(len(lengths)):
        r0, r1 = batch.frame_offsets[i], batch.frame_offsets[i + 1]
        a, b = g[r0:r1, :225].double(), before[1][r0:r1, :225].double()
        rel.append(float(a.abs().max()) if float(b.norm()) == 0.0 else float((a - b).norm() / b.norm()))
    dl = float((losses - before[2]).abs().max())
    print(f"G3 general route against the card route: detect {dv:.1e} (bound 1e-5), first gradient rel L2 per clip "
          f"{['%.1e' % r for r in rel]} (bound 2e-4), five losses {dl:.1e} (bound 1e-3), "
          f"finish max |diff| {float((out - before[3]).abs().max()):.1e}")
    assert dv < 1e-5 and max(rel) < 2e-4 and dl < 1e-3


E2E = {}


def end_to_end(rt, name):
    if name not in E2E:
        from aware_amd.detection import AWAREDetector
        from aware_amd.embedding import AWAREEmbedder
        n_fft, hop, win, window, sr, band, second = GEOM[name]
        emb = AWAREEmbedder(frame_length=n_fft, hop_length=hop, win_length=win, window=window, embedding_bands=band,
                            general_geometry=True, verbose=False, loss="push_extremes", num_iterations=400,
                            detection_net_cfg={"n_fft": n_fft, "sample_rate": sr})
        det = AWAREDetector(emb.detection_net, frame_length=n_fft, hop_length=hop, win_length=win, window=window,
                            embedding_bands=band, general_geometry=True)
        clips = [make_clip(s, second)[0] for s in range(4)]
        bits = np.stack([make_clip(s, second)[1] for s in range(4)])
        E2E[name] = (emb, det, clips, bits, sr, hop)
    return E2E[name]


@pytest.mark.parametrize("name", ["G1", "G4"])
def test_end_to_end(rt, name):
    """Four 1 s make_clip clips, 400 steps through embed_batch (graph-captured steps) and detect_batch: clean BER exactly 0,
    mean |value| >= 0.15 (the CPU restatement reads 0.208 at G1 and 0.257 at G4, unmarked audio 0.017-0.021), outputs of
    hop * (T - 1) samples."""
    emb, det, clips, bits, sr, hop = end_to_end(rt, name)
    outs = emb.embed_batch(clips, sr, 2.0 * bits - 1.0)
    assert [int(o.numel()) for o in outs] == [hop * (len(c) // hop) for c in clips]
    vals = det.detect_batch([o.cpu().numpy() for o in outs], sr).cpu().numpy()
    ber = float(np.mean((vals > 0).astype(np.int32) != bits) * 100)
    print(f"{name}: clean BER {ber} %, mean |value| {float(np.abs(vals).mean()):.3f}")
    assert ber == 0.0 and float(np.abs(vals).mean()) >= 0.15


@pytest.mark.parametrize("name", ["G1", "G4"])
def test_pipeline(rt, name):
    """WatermarkPipeline.run with such an embedder and detector and PCMBitDepthConversion(16): BER 0 clean and attacked."""
    from aware_amd.attacks import PCMBitDepthConversion
    from aware_amd.pipeline import WatermarkPipeline
    emb, det, clips, bits, sr, hop = end_to_end(rt, name)
    audio = rt.Ragged.from_list(clips)
    res = WatermarkPipeline(emb, det, [PCMBitDepthConversion(16)], sample_rate=sr).run(audio, torch.from_numpy(bits).cuda())
    assert res.watermarked.lengths == [hop * (len(c) // hop) for c in clips]
    assert int(res.clean_bit_errors) == 0 and int(res.bit_errors) == 0


def test_through_load(rt, tmp_path):
    """A card with general_geometry: true (G4's framing at 44.1 kHz) through load(): embed and detect, a short run."""
    from aware_amd.utils.models import load
    card = tmp_path / "card.yaml"
    card.write_text("frame_length: 2048\nhop_length: 512\nwin_length: 2048\ngeneral_geometry: true\nnum_iterations: 40\n"
                    "detection_net_cfg: {sample_rate: 44100, n_fft: 2048}\nloss: push_extremes\nverbose: false\n")
    emb, det = load(str(card))
    clip, bits = make_clip(1, 44100)
    y = emb.embed(clip, 44100, 2.0 * bits - 1.0)
    assert y.shape == (512 * (44100 // 512),) and np.isfinite(y).all()
    vals = det.detect(y, 44100)
    assert vals.shape == (20,) and float(np.abs(vals).mean()) > float(np.abs(det.detect(clip, 44100)).mean())


def test_registry_optimizer_on_the_general_route(rt):
    """A registry optimiser with a schedule (Adam, cosine: launch_opt_rows on the gradient band_coef_grad leaves) at G1
    against the restatement's torch.optim loop, per-step losses to 1e-3 (the bound of tests/test_gpu_wide_band.py)."""
    from aware_amd.embedding import AWAREEmbedder
    n = 6
    n_fft, hop, win, window, sr, band, second = GEOM["G1"]
    emb = AWAREEmbedder(frame_length=n_fft, hop_length=hop, win_length=win, general_geometry=True, num_iterations=n,
                        verbose=False, use_graph=False, loss="push_extremes", detection_net_cfg={"n_fft": n_fft},
                        optimizer_cfg={"name": "adam", "params": {"lr": 0.05}},
                        scheduler_cfg={"name": "cosine_annealing", "params": {"T_max": n}})
    audio, bits = make_clip(3, second)
    wm = (2 * bits - 1).astype(np.float32)
    batch = emb.make_batch([second], sr)
    sess = emb.start_session(batch, sr)
    sess.begin(batch.pack([audio]), torch.from_numpy(wm)[None].cuda())
    mine = []
    for _ in range(n):
        sess.iterate(1)
        mine.append(float(sess.loss.cpu()[0]))
    ref = []
    loop32("G1", num_iterations=n, optimizer="adam", optimizer_params={"lr": 0.05}, scheduler="cosine_annealing",
           scheduler_params={"T_max": n}).embed_registry(audio[None], wm[None], record=lambda it, l, lr: ref.append(l))
    assert np.abs(np.asarray(mine) - np.asarray(ref)).max() < 1e-3, (mine, ref)


def test_errors(rt):
    """A workspace one byte short is AWARE_E_WORKSPACE (the carve is exact); a general batch with a plan of another geometry
    is AWARE_E_BADARG; a detector made for another plan is AWARE_E_BADARG."""
    from aware_amd._lib import EmbedConfig
    c, other = case(rt, "G1"), case(rt, "G2")
    lib, plan, dev, batch = c["plan"].lib, c["plan"], c["dev"], c["batch"]
    audio = batch.pack(c["clips"])
    vals = torch.empty((batch.B, 20), device="cuda")
    nbytes = lib.aware_detect_workspace_bytes(batch.h, dev.h)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    args = (C.c_void_p(audio.data_ptr()), C.c_void_p(vals.data_ptr()), C.c_void_p(ws.data_ptr()))
    assert lib.aware_detect(plan.h, dev.h, batch.h, *args, nbytes, None) == 0
    assert lib.aware_detect(plan.h, dev.h, batch.h, *args, nbytes - 1, None) == -4
    assert lib.aware_detect(other["plan"].h, dev.h, batch.h, *args, nbytes, None) == -1
    assert lib.aware_detect(plan.h, other["dev"].h, batch.h, *args, nbytes, None) == -1
    card = rt.Plan()
    assert lib.aware_detect(card.h, dev.h, batch.h, *args, nbytes, None) == -1
    # the same geometry without the flag AWARE_PLAN_GENERAL is a plan for the transforms alone
    plain = rt.Plan(*GEOM["G1"][:4], band_bins=plan.band_bins)
    assert plain.general and lib.aware_detect(plain.h, dev.h, batch.h, *args, nbytes, None) == -2
    sess = rt.EmbedSession(plan, dev, batch, num_iterations=2, use_graph=False)
    cfg, h = sess.cfg, C.c_void_p()
    big = torch.empty(sess.nbytes, dtype=torch.uint8, device="cuda")
    assert lib.aware_embed_create(C.byref(h), plan.h, dev.h, batch.h, C.byref(cfg), C.c_void_p(big.data_ptr()), sess.nbytes - 1, None) == -4
    assert lib.aware_embed_create(C.byref(h), other["plan"].h, dev.h, batch.h, C.byref(cfg), C.c_void_p(big.data_ptr()), sess.nbytes, None) == -1
    assert lib.aware_embed_create(C.byref(h), plan.h, dev.h, batch.h, C.byref(cfg), C.c_void_p(big.data_ptr()), sess.nbytes, None) == 0
    lib.aware_embed_destroy(h)
    l1 = EmbedConfig.from_buffer_copy(cfg)
    l1.loss = rt.LOSS_KINDS["push_extremes_l1"]
    assert lib.aware_embed_create(C.byref(h), plan.h, dev.h, batch.h, C.byref(l1), C.c_void_p(big.data_ptr()), sess.nbytes, None) == -2
    torch.cuda.synchronize()


def test_refusals_on_the_device(rt):
    """The refusals of the host file hold with a GPU present too: nothing is launched for them."""
    c = case(rt, "G1")
    clip = [c["clips"][0]]
    for feature, fn in (("sync_search", lambda: c["det"].detect_batch(clip, 16000, sync_search=8)),
                        ("speed_search", lambda: c["det"].detect_batch(clip, 16000, speed_search=5.0)),
                        ("scan", lambda: c["det"].scan(clip, 16000))):
        with pytest.raises(NotImplementedError, match=feature) as exc:
            fn()
        assert "general_geometry" in str(exc.value)
    sess = rt.EmbedSession(c["plan"], c["dev"], c["batch"], num_iterations=2, use_graph=False)
    with pytest.raises(Exception, match="unsupported"):
        sess.set_loop_attacks([{"kind": "gaussian_noise", "snr_db": 10.0}], [0] * c["batch"].B)
