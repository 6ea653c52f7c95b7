"""GPU tests of embed and detect on clips longer than 10.24 s, against the CPU oracle (oracle/aware_oracle.py) and the
float64 restatement of the detector (test_detector_variants_host.VariantDetector).  Dispatch goes by the longest clip of a
batch, so one long clip moves every clip of its batch onto the branches below; none of them ran in the suite before.

  branch (condition on the batch)                                          pinned by
  ------------------------------------------------------------------------------------------------------------------------
  T >= 642: last card block Conv::Plain instead of SplitK, read-out        test_first_iteration_long[b, c, d], test_detect_long,
    head_kernel, backward through launch_norm_act and a plain                test_trajectory_20_steps_graph
    data-gradient GEMM with K = 40 (det_plan)
  pooled > 320: norm_act_{fwd,bwd}_kernel<NORM, ACT, 0> (from memory),     test_first_iteration_long[b, c, d];
    for the card's blocks and for the variants                               test_detector_entry_points_long, test_smooth_variants_embed_gradient_long
  pooled == 320 (T = 641): tail_kernel<., 80> and                          test_first_iteration_long[a]
    norm_act_*_kernel<Instance, LeakyReLU, 80>, every register slot in use
  T = 192 / 193 and pooled 128 / 129: clip form <-> chunked form of the    test_first_iteration_long[e, f]
    mel norm (kMelClipFrames), clip_tile_groups 4 -> 0
  T >= 65 536: no flat workgroup table, (runs, B) grids of the stream      test_stft_and_detect_at_the_workgroup_table_limit
    kernels, analysis run length 16
  any long clip: more than 4 chunks in the ragged conv and read-out        test_first_iteration_long[d] (7 chunks),
    gradient kernels, readout_wide_kernel's time loop, chunked mel           test_detector_entry_points_long[card64], test_stft_long_batch
    partials, peak partials with pstride > 40
  one pooled frame next to a long clip: the from-memory backward kernels     test_first_iteration_long[c] (failed on the f32 pipe
    must leave its gradient exactly 0                                          before mul_rounded), test_one_pooled_frame_in_a_long_batch_variant

Kinks.  The loss is not differentiable where a LeakyReLU / ReLU argument is 0; within rounding of 0 the reference's sign is
decided by rounding as much as the kernel's.  The older first-iteration tests relax the gradient bar there, and on long clips
nearly every seed is there.  This module never relaxes: the seeds below were found on the CPU (make_clip / band_mags, an
ascending search for a kink distance that clears the threshold), every test asserts the distance before it compares a
gradient, and every gradient is held to its tight bar.

  card detector, float32 oracle, threshold KINK_CARD = 2e-6 (test_gpu_kernels' threshold), seeds with distance > 4e-6:
    n 48 896 / 49 152 seed 700 (2.1e-5 / 7.0e-6); 65 536 / 65 792 seed 703 (6.4e-6 / 9.0e-6); 65 792 seeds 704, 706 (9.0e-6,
    5.1e-6); 163 840 seed 700 (4.9e-6); 164 096 seeds 701, 736 (4.4e-6, 7.0e-6); 164 369 seed 760 (6.3e-6); 320 000 seed 842
    (6.2e-6); 16 000 seed 1 (8.1e-6); 23 456 seed 2 (5.1e-6); 100 001 seed 14 (7.1e-6)
  detector entry points, float64 restatement, threshold KINK = 1e-5 (the variants tests' threshold): MAG_SEEDS below; three
    clips that no seed carries that far: KINK_FLOOR below.
  The float32 oracle's distances move with the CPU it runs on (320 000 / 842: 6.2e-6 and 4.8e-6 on two machines); that is what
  the factor 2 between search and assertion is for.

Measured on MI355X (every figure is printed before it is asserted; maxima over clips, pipes and batches):
  test_first_iteration_long (18 cases + staged DSP): loss 1.2e-7 (bar 2e-5), prediction 3.0e-7 (bar 5e-5), gradient
    1.7e-6 ... 2.4e-6 relative L2 (bar 5e-5; the 320 000-sample clip 2.2e-6 ... 2.4e-6), the 513-sample clip's gradient 0
  test_detect_long: 2.4e-7 (bar 5e-5)
  test_detector_entry_points_long: values 2.5e-7 (bar 5e-5), gradients 7.3e-7 ... 2.7e-6 (bar 1e-4)
  test_smooth_variants_embed_gradient_long: loss 1.2e-7, prediction 1.9e-7, gradients 1.5e-6 ... 3.3e-6 (bar 1e-4)
  test_trajectory_20_steps_graph: step 0 exact, 20 steps 1.0e-3 (bar 3.6e-3), detect of the output 2.7e-7 (bar 5e-5)
  test_stft_long_batch: STFT / band 2.3e-7 (bar 1e-5), iSTFT and round trip 3.0e-7 (bar 2e-6), unit peak exact, both
    backward transforms 2.1e-7 (bar 2e-6)
  test_stft_and_detect_at_the_workgroup_table_limit: STFT / band 2.3e-7, iSTFT 3.6e-7, detect 1.2e-6 (T = 65 536) and
    1.0e-6 (T = 65 535) against a bar of 5e-5
No bar was raised: the reference-yardstick fallback (float32 against float64 oracle) was not needed anywhere.
A kernel trace of this module shows head_kernel<4>, norm_act_{fwd,bwd}_kernel<0|1|2, ., 0, false> (the card's blocks at
<0, 1, 0, false>), readout_wide_kernel<4, 2>, tail_kernel<4, 80>, norm_act_*_kernel<0, 1, 80, false> and analysis_stream_kernel on 1024 x 1
workgroups (run length 16, T = 65 536) next to 1366 from the table (run length 12, T = 65 535).
"""
import numpy as np
import pytest
import torch

from conftest import make_clip
from test_gpu_kernels import _min_kink_distance, _oracle_first_iteration  # noqa: F401  (_min_kink_distance: inside the latter)
from test_detector_variants_host import VariantDetector, push_extremes_sum
from test_gpu_detector_variants import KINK, band_mags, check_gradient, make_net as make_variant
from test_gpu_detector_variants import oracle_first_iteration as variant_first_iteration
from test_gpu_detector_sizes import band_rows, make_net as make_sized, payload

pytestmark = pytest.mark.gpu

KINK_CARD = 2e-6

# lengths, make_clip seeds (the 513-sample clip has one pooled frame: zero gradient, any seed)
BATCHES = {
    "a": ([163840], [700]),                                                          # T 641, 320 pooled
    "b": ([164096], [701]),                                                          # T 642, 321 pooled
    "c": ([164369, 16000, 164096, 23456, 100001, 513], [760, 1, 736, 2, 14, 3]),     # T 643 (odd, n % 256 != 0) + short clips
    "d": ([320000, 16000], [842, 1]),                                                # 625 pooled: 7 ragged chunks
    "e": ([48896, 49152, 65536, 65792], [700, 700, 703, 703]),                       # T 192, 193, 257, 258
    "f": ([65792] * 3, [703, 704, 706]),                                             # uniform, 129 pooled: ragged kernels
}


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
    return rt.Plan()


@pytest.fixture(scope="module")
def det(rt, plan, O):
    ws, bs = O.detector_weights()
    return rt.DetectorWeights(plan, O.mel_filter_bank(), [w.numpy() for w in ws], [b.numpy() for b in bs])


_CARD_REF = {}


def card_reference(O, seed, n):
    """Clip, payload and the float32 oracle's first iteration (loss, prediction, dL/dcoef [225, T], kink distance) of
    make_clip(seed, n): computed once, shared by every test, never modified."""
    if (seed, n) not in _CARD_REF:
        if "emb" not in _CARD_REF:
            _CARD_REF["emb"] = O.Embedder()
        clip, bits = make_clip(seed, n)
        wm = O.bits_to_bipolar(bits).astype(np.float32)
        if n // 256 < 3:
            # three frames, one pooled frame: the oracle's second STFT refuses the 512 samples its iSTFT returns (reflect
            # padding needs more), and needs no run: InstanceNorm over one frame is 0 in every block, so the prediction is
            # tanh(0) = 0, the loss mean((0 - t)^2) = 1 for a bipolar payload, and the gradient 0
            ref = (1.0, np.zeros(wm.shape[0], np.float32), None, None)
        else:
            ref = _oracle_first_iteration(O, _CARD_REF["emb"], clip, wm)
        _CARD_REF[(seed, n)] = (clip, wm) + ref
    return _CARD_REF[(seed, n)]


def check_first_iteration(rt, plan, det, O, lengths, seeds, **session):
    refs = [card_reference(O, s, n) for s, n in zip(seeds, lengths)]
    batch = rt.Batch(lengths)
    sess = rt.EmbedSession(plan, det, batch, use_graph=False, **session)
    sess.begin(batch.pack([r[0] for r in refs]), torch.from_numpy(np.stack([r[1] for r in refs])).cuda())
    g = sess.gradient()
    torch.cuda.synchronize()
    g = g.cpu()
    loss, pred = sess.loss.cpu().numpy(), sess.pred.cpu().numpy()
    figures = []
    for i, (_, _, l, p, ref, kink) in enumerate(refs):
        mine = g[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :225].T
        el, ep = abs(loss[i] - l), float(np.max(np.abs(pred[i] - p)))
        if batch.frames[i] // 2 == 1:                # one pooled frame: zero variance in every block, zero gradient
            rel = float(mine.abs().max())
            print(f"clip {i} (n = {lengths[i]}): loss err {el:.1e}, pred err {ep:.1e}, max |gradient| {rel:.1e} (must be 0)")
        else:
            rel = (mine - ref).norm().item() / ref.norm().item()
            print(f"clip {i} (n = {lengths[i]}, {batch.frames[i] // 2} pooled frames): loss err {el:.1e}, pred err {ep:.1e}, "
                  f"gradient rel L2 {rel:.2e}, kink {kink:.1e}")
        figures.append((el, ep, rel))
    worst = np.max(np.asarray(figures), axis=0)
    print(f"max over the batch: loss {worst[0]:.1e} (bar 2e-5), pred {worst[1]:.1e} (bar 5e-5), gradient {worst[2]:.2e} (bar 5e-5)")
    assert bool(torch.isfinite(g).all())
    for i, (el, ep, rel) in enumerate(figures):
        assert el < 2e-5, (i, el)
        assert ep < 5e-5, (i, ep)
        if batch.frames[i] // 2 == 1:
            assert rel == 0.0, (i, rel)
        else:
            assert refs[i][5] > KINK_CARD, (i, lengths[i], seeds[i], refs[i][5])
            assert rel < 5e-5, (i, rel, refs[i][5])


@pytest.mark.parametrize("pipe", ["f16x2", "bf16x3", "f32"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_first_iteration_long(rt, plan, det, O, name, pipe):
    """Loss, prediction and dL/dcoef of the first loop body on the card detector at the dispatch boundaries, against torch
    autograd on the float32 oracle: loss 2e-5, prediction 5e-5, gradient 5e-5 relative L2 for every clip, every clip clear
    of a kink.  In (c) and (d) the short clips run on the long-clip kernels (head_kernel, norm_act_* from memory, chunked
    mel norm) and are held to the same bars.  The 513-sample clip has one pooled frame: its gradient is exactly zero."""
    check_first_iteration(rt, plan, det, O, *BATCHES[name], conv_pipe=pipe)


def test_first_iteration_long_staged_dsp(rt, plan, det, O):
    """Batch (c) once more on the workgroup-staged STFT / iSTFT kernels."""
    check_first_iteration(rt, plan, det, O, *BATCHES["c"], dsp_path="staged")


@pytest.mark.parametrize("name", ["c", "d"])
def test_detect_long(rt, plan, det, O, name):
    """aware_detect (readout_forward -> launch_head) against the oracle's detect_raw, per clip, atol 5e-5."""
    lengths, seeds = BATCHES[name]
    clips = [card_reference(O, s, n)[0] for s, n in zip(seeds, lengths)]
    batch = rt.Batch(lengths)
    vals = rt.detect(plan, det, batch, batch.pack(clips)).cpu().numpy()
    emb = O.Embedder()
    err = [float(np.max(np.abs(vals[i] - emb.detect_raw(c[None])[0].numpy()))) for i, c in enumerate(clips)]
    print(f"batch ({name}): max |detect - detect_raw| per clip {['%.1e' % e for e in err]} (bar 5e-5)")
    assert np.isfinite(vals).all() and max(err) < 5e-5, err


# band_mags seed per clip (frames 642, 63, 1251) and the float64 kink distance it gives; smooth networks have no kink
MAG_SEEDS = {
    "gelu_instance_tanh": (0, 1, 2),
    "swish_batch_tanh": (0, 1, 2),
    "m13_odd": (0, 0, 0),                        # 1.5e-5, 2.1e-4, 2.8e-5
    "card64": (1632, 0, 216261),                 # 1.2e-5, 4.4e-5, 8.7e-6 (*)
    "relu_none_sigmoid": (892, 49, 64278),       # 3.1e-6 (*), 1.4e-5, 2.1e-6 (*)
}
ENTRY_FRAMES = [642, 63, 1251]
# (*) No seed reaches KINK = 1e-5 on these three clips.  The smallest |u| of a clip is the minimum over all block arguments, of
# which the card's widths have 1.7 M at 625 pooled frames, and without a norm layer they crowd around 0.  Measured on the CPU,
# smallest |u| per seed: card64 at 1251 frames mean 8.4e-7 over 150 seeds, largest 8.7e-6 over 200 000 seeds; relu_none at 642
# frames mean 3.8e-7, largest 3.1e-6 over 3000; at 1251 frames mean 1.9e-7, largest 2.1e-6 over 120 000.  With the minimum
# exponentially distributed at those means a seed clears 1e-5 with probability e^-12, e^-26 and e^-52.  These clips are asserted
# against KINK_CARD = 2e-6 instead, the threshold of the first-iteration tests above for the same question (f32 rounding of
# u is ~1e-7), and their gradients are held to the same tight bar as every other clip; none is compared at a looser one.
KINK_FLOOR = {("card64", 1251): KINK_CARD, ("relu_none_sigmoid", 642): KINK_CARD, ("relu_none_sigmoid", 1251): KINK_CARD}


def entry_net(name):
    if name == "m13_odd":
        return make_sized(name)
    if name == "card64":                       # the card's architecture and widths with a 64-bit payload: 128 read-out channels
        return make_sized("m64_L64", n_mels=128)
    return make_variant(name)


@pytest.mark.parametrize("name", list(MAG_SEEDS))
def test_detector_entry_points_long(rt, name):
    """aware_detector_forward / _backward on band magnitudes of 642, 63 and 1251 frames against the float64 restatement:
    values to 5e-5, the push_extremes magnitude gradient per clip to 1e-4 relative L2, every clip clear of a kink (by KINK,
    or by KINK_FLOOR where no seed reaches that).  The smooth networks cover norm_act_*_kernel<Instance / Affine, ., 0>,
    relu_none the element-wise norm, m13_odd the chunked mel norm on MelBankAny (mel_*_kernel<MelBankAny>) and odd widths, card64 readout_wide_kernel over
    625 pooled frames."""
    from aware_amd.utils.audio import default_plan
    plan = default_plan()
    net = entry_net(name)
    L = net.output_length
    dev = net.device_weights(plan)
    assert dev.is_card == net.is_card_arch
    batch = rt.Batch([164096, 16000, 320000])
    assert batch.frames == ENTRY_FRAMES
    mags = [band_mags(np.random.default_rng(s), [T])[0] for s, T in zip(MAG_SEEDS[name], ENTRY_FRAMES)]
    rows = band_rows(rt, batch, mags)
    target = torch.from_numpy(payload(L, batch.B, L))
    vals = rt.detector_forward(plan, dev, batch, rows)
    assert tuple(vals.shape) == (batch.B, L)
    p = vals.detach().clone().requires_grad_(True)
    push_extremes_sum(p, target.cuda()).backward()
    vals2, gmag = rt.detector_backward(plan, dev, batch, rows, p.grad)
    vals, vals2, gmag = vals.cpu().numpy(), vals2.cpu().numpy(), gmag.cpu().numpy()
    np.testing.assert_allclose(vals, vals2, rtol=0, atol=1e-6)
    assert np.isfinite(gmag).all()
    vd = VariantDetector(net)
    figures = []
    for i, m in enumerate(mags):
        x = torch.from_numpy(m).double()[None].requires_grad_(True)
        ref = vd.forward(x)
        push_extremes_sum(ref, target[i:i + 1].double()).backward()
        ev = float(np.max(np.abs(vals[i] - ref.detach().numpy()[0])))
        kink = vd.kink_distance(x.detach())[0]
        mine = gmag[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :225].T
        gref = x.grad.numpy()[0, 32:257]
        rel = float(np.linalg.norm(mine - gref) / np.linalg.norm(gref))
        floor = KINK_FLOOR.get((name, ENTRY_FRAMES[i]), KINK)
        print(f"{name} clip {i} (T {batch.frames[i]}): value err {ev:.1e} (bar 5e-5), gradient rel L2 {rel:.2e} (bar 1e-4), "
              f"kink {kink:.1e} (above {floor:.0e})")
        figures.append((i, ev, kink, floor, rel))
    for i, ev, kink, floor, rel in figures:
        assert ev < 5e-5, (name, i, ev)
        assert kink > floor, (name, i, MAG_SEEDS[name][i], kink)
        assert rel < 1e-4, (name, i, rel, kink)


_SMOOTH_REF = {}


@pytest.mark.parametrize("pipe", ["f16x2", "bf16x3", "f32"])
@pytest.mark.parametrize("key", ["gelu_instance_tanh", "swish_batch_tanh"])
def test_smooth_variants_embed_gradient_long(rt, O, key, pipe):
    """The detector entry points run on one conv pipe; the embed loop's first gradient takes the same staged route
    (norm_act_*_kernel<Instance / Affine, ., 0> beyond 320 pooled frames) on all three.  GELU and Swish have no kink, so
    the bars hold unconditionally: loss 2e-5, prediction 5e-5, dL/dcoef 1e-4 relative L2 against float64 autograd."""
    from aware_amd.utils.audio import default_plan
    plan = default_plan()
    net = make_variant(key)
    lengths = [164096, 16000, 320000]
    pairs = [make_clip(900 + i, n) for i, n in enumerate(lengths)]
    wm = np.stack([O.bits_to_bipolar(p[1]) for p in pairs]).astype(np.float32)
    batch = rt.Batch(lengths)
    sess = rt.EmbedSession(plan, net.device_weights(plan), batch, use_graph=False, conv_pipe=pipe)
    sess.begin(batch.pack([p[0] for p in pairs]), torch.from_numpy(wm).cuda())
    g = sess.gradient().cpu().numpy()
    lv, pv = sess.loss.cpu().numpy(), sess.pred.cpu().numpy()
    for i in range(len(lengths)):
        if (key, i) not in _SMOOTH_REF:
            _SMOOTH_REF[(key, i)] = variant_first_iteration(O, net, pairs[i][0], wm[i], "push_extremes")
        l, p, ref, kink = _SMOOTH_REF[(key, i)]
        mine = g[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :225].T
        print(f"{key} {pipe} clip {i}: loss err {abs(lv[i] - l):.1e}, pred err {np.max(np.abs(pv[i] - p)):.1e}")
        assert abs(lv[i] - l) < 2e-5, (i, lv[i], l)
        assert np.max(np.abs(pv[i] - p)) < 5e-5
        assert kink == float("inf")
        check_gradient(mine, ref, kink, f"{key} {pipe} clip {i} (T {batch.frames[i]})", 1e-4)


@pytest.mark.parametrize("pipe", ["f16x2", "f32"])
def test_one_pooled_frame_in_a_long_batch_variant(rt, O, pipe):
    """A 513-sample clip next to a 164 096-sample one on a LeakyReLU + InstanceNorm variant (norm_act_bwd_kernel<Instance,
    LeakyReLU, 0>, the from-memory form): one pooled frame has zero variance in every block, so its gradient is exactly
    zero, as on the card detector in batch (c).  (The two sweeps of the from-memory backward kernels once disagreed on dL/du
    by the rounding of its product with the slope 0.2, and left 1e-25 here.)"""
    from aware_amd.utils.audio import default_plan
    plan = default_plan()
    net = make_variant("leaky_relu_instance_sigmoid")
    lengths = [164096, 513]
    pairs = [make_clip(910 + i, n) for i, n in enumerate(lengths)]
    wm = np.stack([O.bits_to_bipolar(p[1]) for p in pairs]).astype(np.float32)
    batch = rt.Batch(lengths)
    sess = rt.EmbedSession(plan, net.device_weights(plan), batch, use_graph=False, conv_pipe=pipe, loss="push_sigmoid")
    sess.begin(batch.pack([p[0] for p in pairs]), torch.from_numpy(wm).cuda())
    g = sess.gradient().cpu()
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(sess.loss).all())
    assert float(g[: batch.frame_offsets[1]].abs().max()) > 0.0
    assert float(g[batch.frame_offsets[1]:].abs().max()) == 0.0


def test_trajectory_20_steps_graph(rt, plan, det, O):
    """Twenty optimiser steps with graph replay on [164096, 16000]: every step's loss against the oracle's (step 0 to 2e-5,
    every step to 3 x 1.2e-3, test_embed_short_trajectory's bar), then finish(): output lengths 256 (T - 1), finite, and
    aware_detect of the output against the oracle's detect_raw of the same output at 5e-5."""
    lengths, seeds = [164096, 16000], [701, 1]
    refs = [card_reference(O, s, n) for s, n in zip(seeds, lengths)]
    clips, wm = [r[0] for r in refs], np.stack([r[1] for r in refs])
    batch = rt.Batch(lengths)
    sess = rt.EmbedSession(plan, det, batch, num_iterations=20, use_graph=True)
    sess.begin(batch.pack(clips), torch.from_numpy(wm).cuda())
    mine = []
    for _ in range(20):
        sess.iterate(1)
        mine.append(sess.loss.cpu().numpy().copy())
    mine = np.stack(mine)
    assert int(sess.step.cpu()[0]) == 20
    out = sess.finish(torch.tensor([float(np.max(c)) for c in clips], device="cuda"))
    torch.cuda.synchronize()
    assert batch.out_lengths == [256 * (T - 1) for T in batch.frames]
    outs = [o.cpu().numpy() for o in batch.unpack_out(out)]
    vals = rt.detect(plan, det, rt.Batch(batch.out_lengths, in_offsets=batch.out_offsets), out).cpu().numpy()
    for i, c in enumerate(clips):
        emb = O.Embedder(num_iterations=20)
        ref = []
        emb.embed(c[None], wm[i][None], record=lambda it, l, p, g: ref.append(float(l[0])))
        d = np.abs(mine[:, i] - np.asarray(ref))
        assert outs[i].shape == (256 * (batch.frames[i] - 1),) and np.isfinite(outs[i]).all()
        ed = float(np.max(np.abs(vals[i] - emb.detect_raw(outs[i][None])[0].numpy())))
        print(f"clip {i} (n = {lengths[i]}): |loss - oracle| step 0 {d[0]:.1e} (bar 2e-5), max over 20 steps {d.max():.1e} "
              f"(bar 3.6e-3); detect of the output vs detect_raw {ed:.1e} (bar 5e-5)")
        assert d[0] < 2e-5
        assert d.max() < 3 * 1.2e-3, (mine[:, i], ref)
        assert ed < 5e-5


def check_transforms(rt, plan, O, lengths, clips):
    """aware_stft / _istft / _stft_band against the float32 oracle with the bars of test_stft_istft_vs_oracle and
    test_stft_band: spectrum and band 1e-5 of the largest magnitude, inverse and round trip 2e-6, unit peak to 1e-6."""
    batch = rt.Batch(lengths)
    audio = batch.pack(clips)
    spec = rt.stft(plan, batch, audio, normalize=True)
    y = rt.istft(plan, batch, spec, normalize=False).cpu()
    yn = rt.istft(plan, batch, spec, normalize=True).cpu()
    mag, ph = rt.stft_band(plan, batch, audio, normalize=True)
    spec, mag, ph = spec.cpu(), mag.cpu(), ph.cpu()
    worst = [0.0, 0.0, 0.0, 0.0]
    for i, c in enumerate(clips):
        x = O.waveform_normalize(torch.as_tensor(c))
        S = O.stft(x)                                                        # [513, T]
        assert S.shape[1] == batch.frames[i]
        sl = slice(batch.frame_offsets[i], batch.frame_offsets[i + 1])
        top = S.abs().max().item()
        es = (spec[sl, :513].T - S).abs().max().item() / top
        eb = max((mag[sl, :225].T - S[32:257].abs()).abs().max().item(),
                 ((mag[sl, :225] * ph[sl, :225]).T - S[32:257]).abs().max().item()) / top
        assert mag[sl, 225:].abs().max().item() == 0.0
        ref = O.istft(S)
        seg = y[batch.out_offsets[i]: batch.out_offsets[i] + batch.out_lengths[i]]
        assert seg.shape == ref.shape
        ei = max((seg - ref).abs().max().item(), (seg - x[: seg.shape[0]]).abs().max().item())
        ep = abs(yn[batch.out_offsets[i]: batch.out_offsets[i] + batch.out_lengths[i]].abs().max().item() - 1.0)
        del S, ref
        print(f"clip {i} (n = {lengths[i]}, T = {batch.frames[i]}): stft {es:.1e}, band {eb:.1e} (bars 1e-5), istft / round trip "
              f"{ei:.1e} (bar 2e-6), unit peak {ep:.1e} (bar 1e-6)")
        assert es < 1e-5 and eb < 1e-5, (i, es, eb)
        assert ei < 2e-6, (i, ei)
        assert ep < 1e-6, (i, ep)
        worst = [max(a, b) for a, b in zip(worst, (es, eb, ei, ep))]
    return worst


def test_stft_long_batch(rt, plan, O):
    """STFT, band STFT, iSTFT and the two backward transforms on [164133, 320000, 513, 16000] (chunked peak partials, a
    length that is no multiple of the hop, the shortest legal clip): forward against the float32 oracle, aware_stft_bwd and
    aware_istft_bwd against torch autograd on the oracle's explicit restatement (2e-6, as test_stft_backward_any_length
    and test_stft_backward_2d_and_istft_backward)."""
    lengths = [164133, 320000, 513, 16000]
    clips = [make_clip(10 + i, n)[0] for i, n in enumerate(lengths)]
    check_transforms(rt, plan, O, lengths, clips)
    batch = rt.Batch(lengths)
    g = torch.Generator().manual_seed(sum(lengths))
    G = torch.zeros((batch.total_frames, rt.FULL_STRIDE), dtype=torch.complex64)
    G[:, :513] = torch.complex(torch.randn(batch.total_frames, 513, generator=g), torch.randn(batch.total_frames, 513, generator=g))
    ga = rt.stft_bwd(plan, batch, G.cuda()).cpu()
    w = torch.randn(batch.total_out, generator=g)
    gs = rt.istft_bwd(plan, batch, w.cuda()).cpu()
    assert ga.shape[0] == sum(lengths)
    for i, c in enumerate(clips):
        sl = slice(batch.frame_offsets[i], batch.frame_offsets[i + 1])
        x = torch.from_numpy(c).clone().requires_grad_(True)
        S = O.stft(x[None])[0]
        Gi = G[sl, :513].T
        (S.real * Gi.real + S.imag * Gi.imag).sum().backward()
        rel = float((ga[batch.in_offsets[i]: batch.in_offsets[i] + lengths[i]] - x.grad).norm() / x.grad.norm())
        X = S.detach().to(torch.complex128).requires_grad_(True)
        wi = w[batch.out_offsets[i]: batch.out_offsets[i] + batch.out_lengths[i]]
        (O.istft(X) * wi.double()).sum().backward()
        ri = float((gs[sl, :513].T.to(torch.complex128) - X.grad).abs().max() / X.grad.abs().max())
        print(f"clip {i} (n = {lengths[i]}): stft_bwd rel L2 {rel:.1e}, istft_bwd max err / max {ri:.1e} (bars 2e-6)")
        assert rel < 2e-6, (i, rel)
        assert ri < 2e-6, (i, ri)


def test_stft_and_detect_at_the_workgroup_table_limit(rt, plan, det, O):
    """One clip of 16 776 960 samples (T = 65 536: the batch builds no flat workgroup table, the stream kernels launch on a
    (runs, B) grid, the analysis at run length 16) and one of 16 776 959 (T = 65 535, the longest with the table): STFT,
    band STFT, iSTFT and round trip against the float32 oracle, aware_detect against detect_raw at 5e-5."""
    emb = O.Embedder()
    for n in (16776960, 16776959):
        clip = (0.1 * np.random.default_rng(n).standard_normal(n)).astype(np.float32)
        batch = rt.Batch([n])
        assert batch.frames == [1 + n // 256]
        worst = check_transforms(rt, plan, O, [n], [clip])
        vals = rt.detect(plan, det, batch, batch.pack([clip])).cpu().numpy()[0]
        ed = float(np.max(np.abs(vals - emb.detect_raw(clip[None])[0].numpy())))
        print(f"n = {n} (T = {batch.frames[0]}): stft {worst[0]:.1e}, band {worst[1]:.1e}, istft {worst[2]:.1e}, detect vs "
              f"detect_raw {ed:.1e} (bar 5e-5)")
        assert np.isfinite(vals).all() and ed < 5e-5, ed
        del clip, batch
        torch.cuda.empty_cache()
