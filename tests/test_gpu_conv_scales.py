"""The per-clip power-of-two scales of the f16 two-term conv pipe (gemm_h2.hip through conv_block.hpp) on batches whose
clips differ in amplitude by many binades: at the GEMM (every scale edge, every epilogue, the partial maxima it leaves) and
through the embed loop and detection, where the maxima come from the in-loop producers (mel kernels, conv epilogues, read-out,
the clip_amax / ragged_amax hand-over pre-passes).

Run on the MI355X box:  python -m pytest tests/test_gpu_conv_scales.py -m gpu -q -s
"""
import time

import numpy as np
import pytest
import torch

from conftest import make_clip

pytestmark = pytest.mark.gpu


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


def _block_reference(a, w, bias, act, rstd, B, RP, Tp, epi):
    """fp64 restatement of one Conv1dBlock (detection/modules/conv1d.py:38-42) / of its backward (as test_gpu_kernels.py)."""
    N = w.shape[0]
    z = (a.double() @ w.double().T).view(B, RP, N)[:, :Tp]
    if epi == 0:
        return z + bias.double()
    if epi == 1:
        z = z + bias.double()
        u = (z - z.mean(1, keepdim=True)) / torch.sqrt(z.var(1, unbiased=False, keepdim=True) + 1e-5)
        return torch.where(u > 0, u, 0.2 * u)
    av = act.double().view(B, RP, N)[:, :Tp]
    u = torch.where(av > 0, av, av * 5.0)
    du = z * torch.where(av > 0, 1.0, 0.2)
    return rstd.double()[:, None, :] * (du - du.mean(1, keepdim=True) - u * (du * u).mean(1, keepdim=True))


# ---------------------------------------------------------------------------------------------------------
# 1. GEMM level: one uniform batch, one clip per scale edge
# ---------------------------------------------------------------------------------------------------------
FLT_MIN = 2.0 ** -126
# clip -> (kind, log2 of its maximum).  Every other clip: randn times 2^[-6, 4).
EDGE_CLIPS = {0: ("zero", None), 1: ("single", -0.415), 2: ("pow2", 3), 3: ("ulp_below_pow2", 4), 4: ("pow2", -20),
              5: ("scaled", 100), 6: ("scaled", -100), 7: ("scaled", -109), 8: ("scaled", -118), 9: ("pow2", -124),
              10: ("scaled", -130), 11: ("scaled", -140), 12: ("last_group", 3.3), 13: ("pow2", -107)}
# weight rows with small maxima (the detector's rows are O(1); these meet the tiny clips above: 2^-sa * binv underflows)
EDGE_ROWS = {3: -20, 17: -40, 100: -60, 130: -80, 260: -100, 511: -110}


def _edge_operands(B, RP, Tp, N, K, epi, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, RP, K, generator=g, dtype=torch.float64)
    a *= torch.exp2(torch.randint(-6, 4, (B, 1, 1), generator=g).double())
    for clip, (kind, e) in EDGE_CLIPS.items():
        x = torch.randn(RP, K, generator=g, dtype=torch.float64)
        if kind == "zero":
            x.zero_()
        elif kind == "single":
            x.zero_()
            x[Tp // 2, K // 3] = -0.75
        elif kind in ("pow2", "ulp_below_pow2"):
            x = x / x.abs().max() * 0.9 * 2.0 ** e
            x[7, 5] = 2.0 ** e if kind == "pow2" else -float(np.nextafter(np.float32(2.0 ** e), np.float32(0)))
        elif kind == "last_group":
            x = x / x.abs().max() * 2.0 ** (e - 1)
            x[Tp - 1, K - 1] = 2.0 ** e                                    # the clip's maximum: last row, last 16 columns
        else:
            # the variance of an InstanceNorm'd output near 2^100 overflows f32 in every pipe: 2^50 for the normalising epilogues
            if e == 100 and epi != 0 and epi != 2:
                e = 50
            x = x / x.abs().max() * 2.0 ** e
        a[clip] = x
    a[:, Tp:] = 0
    a = a.reshape(B * RP, K).float()
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-4, 3, (N, 1), generator=g).float()) / K ** 0.5
    for row, e in EDGE_ROWS.items():
        w[row] = (w[row].double() / w[row].double().abs().max() * 2.0 ** e).float()
    return a, w


@pytest.mark.parametrize("epi", [0, 1, 2, "last"])
def test_gemm_clip_h2_per_clip_scale_edges(rt, epi):
    """aware_gemm_clip_h2 (gemm_clip_h2_kernel, the production grid: 40 clips x 4 slabs) beside aware_gemm_clip modes 0 (f32
    MFMA) and 1 (bf16x3) on one batch whose clips sit on the edges of h2_scale_for: an all-zero clip, a single non-zero element,
    maxima exactly on and one ulp below a power of two, maxima near 2^100 (2^50 where the InstanceNorm variance would overflow
    f32), 2^-100, in [2^-126, 2^-107) and below 2^-126 (subnormal f32), a maximum in the last row and the last 16 columns; weight
    rows with maxima down to 2^-110.  Against fp64, error relative to the (clip, column) maximum, on every (clip, column) whose
    product A W^T is a normal f32 number: < 4e-6 max(1, K/256) and < 2 e32 + 2e-7 (e32: the f32 MFMA kernel's error on the
    same clip).  The zero clip gives exactly the reference's zeros; no NaN / Inf anywhere; each of the N/16 partial maxima is
    the max |C| of its own 16-column group.  (Before h2_scale_for was capped at 2^126 it returned 1 below 2^-107: the clips in
    that band and every column of the 2^-110 weight row came out as the bias alone, error 1.0.)
    bf16x3 on the same bar for clip maxima >= 2^-107 only (2^-109: 2.6e-6).  Further down it loses precision, as its third
    bf16 term (2^-16 below the value) reaches the subnormal range: measured 6.9e-5 / 9.5e-5 at 2^-118, 5.5e-3 / 6.2e-3 at
    2^-124, 0.37 at 2^-130 (epilogues 0 / 1); printed, not asserted.  Inputs that small never reach the conv blocks of the
    loop, where the InstanceNorm and GlobalStandardize in front of them keep the block inputs above 1e-9 (see below)."""
    B, Tp, N, K, CL = 40, 64, 512, 256, 32
    RP = 32 * ((Tp + 31) // 32)
    e = 1 if epi == "last" else epi
    a, w = _edge_operands(B, RP, Tp, N, K, e, seed=4242 + (3 if epi == "last" else epi))
    g = torch.Generator().manual_seed(99)
    bias = torch.zeros(N) if e == 1 else None
    act = torch.randn(B * RP, N, generator=g) if e == 2 else None
    rstd = torch.rand(B, N, generator=g) + 0.5 if e == 2 else None
    wl = torch.randn(CL, N, generator=g) / N ** 0.5 if epi == "last" else None
    ref = _block_reference(a, w, torch.zeros(N), act, rstd, B, RP, Tp, e)        # [B, Tp, N] fp64
    cuda = lambda t: None if t is None else t.cuda()
    outs = {}
    for mode in (0, 1):
        c, _ = rt.gemm_clip(a.cuda(), w.cuda(), cuda(bias), B, Tp, e, cuda(rstd), cuda(act), mode)
        outs[mode] = c.cpu().view(B, RP, N)
    res = rt.gemm_clip_h2(a.cuda(), w, cuda(bias), B, Tp, e, cuda(rstd), cuda(act), w_last=wl)
    c2, amax = res[0].cpu().view(B, RP, N), res[2].cpu()
    assert bool(torch.isfinite(c2).all()), "f16x2: NaN / Inf in the output"
    assert RP == Tp or c2[:, Tp:].abs().max().item() == 0.0                       # padding rows
    # the zero clip: exactly the reference (0 for PLAIN without bias, BWD, and InstanceNorm of a constant)
    assert torch.equal(c2[0, :Tp].double(), ref[0]), c2[0].abs().max()
    # partial maxima: each of the N/16 is the max |C| of its 16-column group (padding rows hold zeros)
    grp = c2.abs().view(B, RP, N // 16, 16).amax(dim=(1, 3))
    np.testing.assert_array_equal(amax[:, : N // 16].numpy(), grp.numpy())

    # the bar holds where the block's product A W^T is a normal f32 number in the (clip, column): below, the epilogue holds it
    # as a subnormal (f32 itself then has fewer than 24 bits; measured on the 2^-130 clip, InstanceNorm epilogue, whose
    # outputs are normal again after the 1/sqrt(1e-5) of the normalisation: f16x2 3.2e-5, f32 MFMA 5.3e-4)
    prod = (a.double() @ w.double().T).view(B, RP, N)[:, :Tp]
    normal = prod.abs().amax(dim=1, keepdim=True) >= FLT_MIN
    scale = ref.abs().amax(dim=1, keepdim=True).clamp_min(1e-300)                  # [B, 1, N]
    err = {k: torch.where(normal, (v[:, :Tp].double() - ref).abs() / scale, torch.zeros(())).amax(dim=(1, 2))
           for k, v in (("f32", outs[0]), ("x3", outs[1]), ("h2", c2))}
    tol = 4e-6 * max(1.0, K / 256)
    for clip in range(B):
        if clip in EDGE_CLIPS or clip < 16:
            kind = EDGE_CLIPS.get(clip, ("random", None))
            print(f"epi {epi} clip {clip:2d} {kind[0]:>14} 2^{kind[1]}: (clip, column)-relative error f32 MFMA "
                  f"{err['f32'][clip]:.2e} bf16x3 {err['x3'][clip]:.2e} f16x2 {err['h2'][clip]:.2e}; "
                  f"normal columns {int(normal[clip].sum())}/{N}")
    bad = [(c, err["h2"][c].item(), err["f32"][c].item()) for c in range(B)
           if not (err["h2"][c] < tol and err["h2"][c] < 2 * err["f32"][c] + 2e-7)]
    assert not bad, f"f16x2 above the bar on (clip, err, f32 err): {bad}"
    big = [c for c in range(B) if EDGE_CLIPS.get(c, ("random", 0))[1] is None or EDGE_CLIPS.get(c, ("random", 0))[1] >= -107]
    bad = [(c, err["x3"][c].item()) for c in big if not err["x3"][c] < tol]
    assert not bad, f"bf16x3 above the bar on (clip, err): {bad}"
    if epi == "last":
        # the split-K partials of the skinny last conv (always on the bf16 three-term split): their sum is the block output
        # times w_last^T.  Same band as bf16x3 above: measured 1.2e-5 on the 2^-124 clip and 5.7e-4 on the 2^-130 one, printed.
        zsum = res[3].cpu().double().sum(0).view(B, RP, CL)
        assert bool(torch.isfinite(zsum).all())
        zref = ref @ wl.double().T
        zmax = zref.abs().amax(dim=1, keepdim=True)
        ez = torch.where(zmax >= FLT_MIN, (zsum[:, :Tp] - zref).abs() / zmax.clamp_min(1e-300), torch.zeros(())).amax(dim=(1, 2))
        print("last-conv partial-sum error per clip:", " ".join(f"{c}:{ez[c].item():.1e}" for c in range(16)))
        bad = [(c, ez[c].item()) for c in big if not ez[c] < 4e-6 * max(1.0, N / 256) + 8 * err["h2"].max().item()]
        assert not bad, bad


# ---------------------------------------------------------------------------------------------------------
# 2. Loop level: mixed-amplitude batches through every conv-block path
# ---------------------------------------------------------------------------------------------------------
# the special clips: peak amplitude (0: silent).  2^-143 is 64 quanta of the smallest subnormal: the loop's two peak
# normalisations (x / (max|x| + 1e-8), twice in the recomputed magnitude) scale every clip above ~1e-24 back to O(1), so only
# clips this small reach the conv blocks in the linear regime with inputs far below O(1) (measured in check c).
SPECIAL = [0.0, 2.0 ** -143, 2.0 ** -130, 1e-30, 1e-20, 1e-12, 1e-9, 1e6]
SHAPES = {
    # batch: (lengths, slots of the special clips, ordinary clips checked against the fp64 oracle)
    "uniform40": ([48000] * 40, [0, 3, 8, 13, 20, 27, 32, 39], [1, 21]),
    "mixed24": ([48000] * 24, [0, 3, 8, 11, 15, 19, 22, 23], [1, 12]),
    "front192": ([48000] * 192, [0, 3, 64, 100, 127, 150, 190, 191], [1, 101]),
    "ragged": ([16000, 160000, 48000, 23456, 100001, 64000, 32000, 128000, 80000, 112000, 41600, 144000],
               [0, 2, 3, 5, 6, 8, 9, 11], [1, 7]),
}
# "within rounding of the kink", relative: the absolute 2e-6 of test_gpu_kernels.py at an ordinary clip's largest |u| (about 4)
KINK_REL = 5e-7
# The loop's own magnitude |S2| = sqrt(re^2 + im^2) runs on the hardware square root, which reads a subnormal sum of squares
# as zero: bins with |S2| < 2^-63 come out as 0 (hot-path code, left as it is).  A clip is held to the
# fp64 bars of check d when fewer than 0.1 % of its band bins of |S2| lie below that in the fp64 oracle at c0.
MAG_FLOOR = 2.0 ** -63
WEAK_SHARE = 1e-3
_ORACLE = {}                   # (clip key) -> oracle results, shared by the shapes whose clips coincide


def _special_clip(k, n):
    x, bits = make_clip(900 + k, n)
    x = x.astype(np.float64) / np.abs(x).max()
    return (x * SPECIAL[k]).astype(np.float32), bits


def _batches(name):
    lengths, slots, _ = SHAPES[name]
    ctrl = [make_clip(600 + i, n) for i, n in enumerate(lengths)]
    test = list(ctrl)
    for k, s in enumerate(slots):
        test[s] = _special_clip(k, lengths[s])
    return lengths, slots, test, ctrl


def _block_inputs(O, emb, mag2):
    """max |x| at the input of each conv block (oracle forward of a [1, 513, T] magnitude)."""
    det = emb.det
    with torch.no_grad():
        x = det.instance_norm(torch.matmul(det.mel, mag2))
        x = (x - x.mean(dim=(1, 2), keepdim=True)) / (x.std(dim=(1, 2), keepdim=True) + 1e-8)
        x = torch.nn.functional.avg_pool1d(x, 2, 2)
        out, kink = [], float("inf")
        for w, b in zip(det.ws, det.bs):
            out.append(float(x.abs().max()))
            u = det.instance_norm(torch.matmul(w, x) + b[:, None])
            # distance to the LeakyReLU kink RELATIVE to the layer's largest |u| (a clip in the linear regime has every |u|
            # tiny; test_gpu_kernels.py's absolute rule would excuse it everywhere)
            if float(u.abs().max()) > 0:
                kink = min(kink, float(u.abs().min() / u.abs().max()))
            x = torch.nn.functional.leaky_relu(u, 0.2)
    return out, kink


def _oracle(O, key, audio, wm_row):
    """f32 oracle forward (block inputs of the loop and of detection, relative kink distance) and fp64 autograd of the first
    loop body; cached per clip."""
    if key in _ORACLE:
        return _ORACLE[key]
    emb = O.Embedder()
    a = torch.from_numpy(audio)[None]
    with torch.no_grad():
        mag0, phase = emb.analyse(a)
        mag2, _ = emb.recompute_magnitude(mag0, phase)
        mag2 = mag2.clone()
        mag2[:, emb.nonband] = 0.0
        loop_in, kink = _block_inputs(O, emb, mag2)
        x = a / torch.amax(torch.abs(a) + 1e-8, dim=-1, keepdim=True)
        mag = torch.abs(O.stft(x)).clone()
        mag[:, emb.nonband] = 0.0
        det_in, _ = _block_inputs(O, emb, mag)
    e64 = O.Embedder(dtype=torch.float64)
    m64, p64 = e64.analyse(a.double())
    with torch.no_grad():
        s2 = e64.recompute_magnitude(m64, p64)[0][0, e64.band]
        weak, bins = int((s2 < MAG_FLOOR).sum()), s2.numel()
    c0 = m64[:, e64.band].clone().requires_grad_(True)
    l, p = e64.forward_loss(c0, m64, p64, torch.from_numpy(wm_row).double()[None])
    l.sum().backward()
    r = dict(loop_in=loop_in, det_in=det_in, kink=kink, loss=float(l.detach()), pred=p[0].detach().numpy(), grad=c0.grad[0],
             weak=weak, bins=bins)
    _ORACLE[key] = r
    return r


def _first_iteration(rt, plan, det, lengths, clips, wm, pipe):
    batch = rt.Batch(lengths)
    sess = rt.EmbedSession(plan, det, batch, use_graph=False, conv_pipe=pipe)
    sess.begin(batch.pack([c[0] for c in clips]), torch.from_numpy(wm).cuda())
    g = sess.gradient()
    torch.cuda.synchronize()
    return batch, g.cpu(), sess.loss.cpu().numpy().copy(), sess.pred.cpu().numpy().copy()


@pytest.mark.parametrize("name", list(SHAPES))
def test_mixed_amplitude_batch_first_iteration(rt, plan, det, O, name):
    """A batch whose special slots hold a silent clip and clips with peaks 2^-143 .. 1e6, beside a control batch with ordinary
    clips there, through the first loop body on the f16x2, bf16x3 and f32 conv pipes.  Shapes: 40 x 3 s (uniform f16x2 forward
    and backward, two-launch mel block), 24 x 3 s (block 0 and its data gradient on bf16x3, the others on f16x2: the clip_amax
    hand-over), 192 x 3 s (one-launch mel block writing the maxima of x0, fused read-out writing gA), ragged 1-10 s
    (gemm_ragged_h2_kernel, ragged_amax).
      a. every ordinary clip's loss, prediction and gradient are bit-identical between the two batches on each pipe;
      b. the special clips agree across pipes: loss and prediction within 2e-6, gradient within 2e-5 relative L2 unless a
         LeakyReLU argument lies within KINK_REL of its kink relative to its layer's largest |u| (then 2e-2);
      c. the special clips do reach the conv blocks at amplitudes many binades apart (oracle forward, printed): the loop's
         block inputs span >= 2^30 (measured 2^32: the two peak normalisations of the recomputed magnitude bring every clip
         above ~1e-24 back to O(1), so the issue's 2^40 is not reachable through the loop), detection's span >= 2^40;
      d. the f32 pipe against fp64 autograd on the oracle for the special clips and two ordinary ones: loss 2e-5, prediction
         5e-5, gradient 5e-5 relative L2 (kink-aware as in b), the bar of the ordinary clips.  Measured on the CPU, the f32
         oracle against fp64 on the special clips: loss <= 1.4e-7, prediction <= 1.8e-7, gradient <= 1.6e-6 (1.5e-3 on one
         clip next to a kink): the normalisations bring a tiny clip back to O(1) before the mel block or scale the linear
         regime exactly, so the special clips are conditioned like ordinary ones.  A clip with a peak below 1e-20 is held
         to the same bars when fewer than 0.1 % of the band bins of its recomputed magnitude |S2| lie below 2^-63 in the fp64
         oracle at c0 (MAG_FLOOR): 1e-30 and 2^-130 count 0 bins and are asserted, 2^-143 counts about 6 % (839 of 14175 on a
         one-second clip) and is printed with its count -- its synthesis reaches the second analysis near 1e-19, where the
         loop's own sqrt(re^2 + im^2) on the hardware square root reads a subnormal sum of squares as zero (hot-path code,
         left as it is: DESIGN.md section 38).  Up to commit 3c94db7 all three were printed only, 1.25 - 1.27 relative L2
         from fp64 with loss and prediction right: the analysis of the original audio at begin used the same plain form, so
         with x / (max|x| + 1e-8) at about 1e8 p every band bin of a clip with peak p <= 1e-28 was stored as magnitude 0 with
         the default phasor (1, 0) (bins lost, measured: 0.06 % at 1e-26, 4.56 % at 1e-27, 99.81 % at 1e-28, 100 % below;
         first gradient 2.3e-2, 0.21, 1.26, 1.28), and aware_embed_gradient projected on (1, 0) instead of the bins' phases,
         while the out-of-band residual, built from the same magnitudes and phasors, kept the first synthesis and with it
         loss and prediction right.  Begin now decomposes with polar_exact (csrc/polar.hpp); tests/test_gpu_quiet_clips.py
         holds the stage itself;
      e. the silent clip: prediction exactly 0, loss exactly the oracle's (1: push_extremes of a zero prediction), finite
         gradient."""
    t0 = time.time()
    lengths, slots, test, ctrl = _batches(name)
    _, _, sample = SHAPES[name]
    wm_t = np.stack([O.bits_to_bipolar(c[1]) for c in test]).astype(np.float32)
    wm_c = np.stack([O.bits_to_bipolar(c[1]) for c in ctrl]).astype(np.float32)
    ordinary = [i for i in range(len(lengths)) if i not in slots]
    res = {}
    for pipe in ("f16x2", "bf16x3", "f32"):
        batch, g_t, l_t, p_t = _first_iteration(rt, plan, det, lengths, test, wm_t, pipe)
        _, g_c, l_c, p_c = _first_iteration(rt, plan, det, lengths, ctrl, wm_c, pipe)
        sl = [slice(batch.frame_offsets[i], batch.frame_offsets[i + 1]) for i in range(len(lengths))]
        # a. isolation
        for i in ordinary:
            assert l_t[i] == l_c[i] and np.array_equal(p_t[i], p_c[i]), (pipe, i, l_t[i], l_c[i])
            assert torch.equal(g_t[sl[i]], g_c[sl[i]]), (pipe, i, (g_t[sl[i]] - g_c[sl[i]]).abs().max())
        for k, s in enumerate(slots):
            assert bool(torch.isfinite(g_t[sl[s]]).all()) and np.isfinite(l_t[s]) and np.isfinite(p_t[s]).all(), (pipe, k)
        res[pipe] = (g_t.double(), l_t, p_t, sl)
    # oracle work: the special clips and two ordinary ones
    orc = {i: _oracle(O, (lengths[i], 900 + slots.index(i)) if i in slots else (lengths[i], 600 + i), test[i][0], wm_t[i])
           for i in list(slots) + sample}
    # c. the spread of the block inputs
    loop_in = np.array([orc[i]["loop_in"] for i in orc])
    det_in = np.array([orc[i]["det_in"] for i in orc])
    for i in orc:
        amp = SPECIAL[slots.index(i)] if i in slots else "ordinary"
        print(f"{name} clip {i} (peak {amp}): block input max |x| loop {['%.1e' % v for v in orc[i]['loop_in']]} "
              f"detect {['%.1e' % v for v in orc[i]['det_in']]} kink(rel) {orc[i]['kink']:.1e}")
    nz = lambda m: m[m > 0]
    sp_loop = [np.log2(nz(loop_in[:, b]).max() / nz(loop_in[:, b]).min()) for b in range(loop_in.shape[1])]
    sp_det = [np.log2(nz(det_in[:, b]).max() / nz(det_in[:, b]).min()) for b in range(det_in.shape[1])]
    print(f"{name}: log2 spread of the block-input maxima per block: loop {np.round(sp_loop, 1)}, detect {np.round(sp_det, 1)}")
    assert sp_loop[0] >= 30 and sp_det[0] >= 40, (sp_loop, sp_det)
    # b. special clips across pipes
    g0, l0, p0, sl = res["f32"]
    for pipe in ("f16x2", "bf16x3"):
        g4, l4, p4, _ = res[pipe]
        for k, s in enumerate(slots):
            kink = orc[s]["kink"]
            n0 = g0[sl[s]].norm().item()
            rel = (g4[sl[s]] - g0[sl[s]]).norm().item() / n0 if n0 > 0 else g4[sl[s]].norm().item()
            print(f"{name} {pipe} vs f32, special clip {k} (peak {SPECIAL[k]:.1e}, slot {s}): loss {abs(l4[s] - l0[s]):.1e} "
                  f"pred {np.max(np.abs(p4[s] - p0[s])):.1e} gradient rel L2 {rel:.2e} kink(rel) {kink:.1e}")
            assert abs(l4[s] - l0[s]) < 2e-6 and np.max(np.abs(p4[s] - p0[s])) < 2e-6, (pipe, k)
            assert rel < (2e-5 if kink > KINK_REL else 2e-2), (pipe, k, rel, kink)
    # d. the f32 pipe against fp64 (a clip whose own |S2| underflows in the loop: printed only, see MAG_FLOOR and the docstring)
    for i in orc:
        o = orc[i]
        mine = g0[sl[i]][:, :225].T
        rn = o["grad"].norm().item()
        rel = (mine - o["grad"]).norm().item() / rn if rn > 0 else mine.norm().item()
        peak = np.abs(test[i][0]).max()
        sub = 0 < peak < 1e-20 and not o["weak"] < WEAK_SHARE * o["bins"]       # from 1e-20 on a clip is held whatever it counts
        why = f" (fp64 oracle: {o['weak']} of {o['bins']} band bins of |S2| below 2^-63: printed only)" if sub else ""
        print(f"{name} f32 pipe vs fp64, clip {i} peak {peak:.1e}{why}: loss {abs(l0[i] - o['loss']):.1e} "
              f"pred {np.max(np.abs(p0[i] - o['pred'])):.1e} gradient rel L2 {rel:.2e}; |S2| < 2^-63 on {o['weak']} of {o['bins']}")
        if not sub:
            assert abs(l0[i] - o["loss"]) < 2e-5 and np.max(np.abs(p0[i] - o["pred"])) < 5e-5, i
            assert rel < (5e-5 if o["kink"] > KINK_REL else 2e-2), (i, rel, o["kink"])
    # e. the silent clip
    s = slots[SPECIAL.index(0.0)]
    for pipe in res:
        g, l, p, _ = res[pipe]
        assert np.all(p[s] == 0.0) and l[s] == np.float32(orc[s]["loss"]) == 1.0, (pipe, l[s], p[s])
    print(f"{name}: {time.time() - t0:.1f} s")


@pytest.mark.parametrize("name", ["uniform40", "front192"])
def test_mixed_amplitude_batch_graph_replay_and_detect(rt, plan, det, O, name):
    """The batches of test_mixed_amplitude_batch_first_iteration through 20 iterations with graph replay (default pipe): the
    ordinary clips' coefficients and finish() output are bit-identical to the control batch's (a partial maximum left over from
    an earlier iteration or another clip would show); the silent clip's coefficients stay 0 and its output is all zero.  Then
    rt.detect on the same audio: every clip's raw outputs within 5e-5 of the oracle's detect_raw, the ordinary clips
    bit-identical to the control batch."""
    t0 = time.time()
    lengths, slots, test, ctrl = _batches(name)
    ordinary = [i for i in range(len(lengths)) if i not in slots]
    batch = rt.Batch(lengths)
    out = {}
    for tag, clips in (("test", test), ("ctrl", ctrl)):
        wm = np.stack([O.bits_to_bipolar(c[1]) for c in clips]).astype(np.float32)
        sess = rt.EmbedSession(plan, det, batch, use_graph=True)
        audio = batch.pack([c[0] for c in clips])
        sess.begin(audio, torch.from_numpy(wm).cuda())
        sess.iterate(20)
        coef = sess.coef.cpu().clone()
        fin = sess.finish(None).cpu()
        vals = rt.detect(plan, det, batch, audio).cpu().numpy()
        out[tag] = (coef, fin, vals, sess.loss.cpu().numpy().copy())
    coef_t, fin_t, v_t, loss_t = out["test"]
    coef_c, fin_c, v_c, _ = out["ctrl"]
    assert np.isfinite(loss_t).all()
    for i in ordinary:
        fs = slice(batch.frame_offsets[i], batch.frame_offsets[i + 1])
        os_ = slice(batch.out_offsets[i], batch.out_offsets[i] + batch.out_lengths[i])
        assert torch.equal(coef_t[fs], coef_c[fs]), (i, (coef_t[fs] - coef_c[fs]).abs().max())
        assert torch.equal(fin_t[os_], fin_c[os_]), i
        assert np.array_equal(v_t[i], v_c[i]), i
    s = slots[SPECIAL.index(0.0)]
    assert coef_t[batch.frame_offsets[s]: batch.frame_offsets[s + 1]].abs().max().item() == 0.0
    assert fin_t[batch.out_offsets[s]: batch.out_offsets[s] + batch.out_lengths[s]].abs().max().item() == 0.0
    assert bool(torch.isfinite(fin_t).all())
    emb = O.Embedder()
    worst = 0.0
    for i in list(slots) + SHAPES[name][2]:
        ref = emb.detect_raw(test[i][0][None])[0].numpy()
        d = float(np.max(np.abs(v_t[i] - ref)))
        worst = max(worst, d)
        assert d < 5e-5, (i, d)
    print(f"{name}: detect raw vs oracle, worst of the special and sampled clips {worst:.1e}; {time.time() - t0:.1f} s")


def test_last_channel_group_sets_the_gradient_scale(rt, plan, O):
    """A producer leaves K/16 partial maxima per clip and the consumer must reduce all of them.  With the detector's last 16
    output channels of every conv block scaled by 1e-4, those channels' InstanceNorm runs in its linear regime (rstd about 316
    instead of about 1): the gradient dL/dZ in the last 16-column group is then hundreds of times larger than in the others, so
    a consumer that skipped that partial would pick a scale that overflows binary16.  40 x 3 s clips (f16x2 conv blocks and
    data gradients) against the f32 pipe: finite, loss and prediction within 1e-5, gradient within 2e-2 relative L2 per clip
    (printed; the bar only has to separate rounding and kink flips from a wrong scale)."""
    ws, bs = O.detector_weights()
    ws = [w.clone() for w in ws]
    for w in ws[:-1]:
        w[-16:] *= 1e-4
    d = rt.DetectorWeights(plan, O.mel_filter_bank(), [w.numpy() for w in ws], [b.numpy() for b in bs])
    lengths = [48000] * 40
    clips = [make_clip(700 + i, n) for i, n in enumerate(lengths)]
    wm = np.stack([O.bits_to_bipolar(c[1]) for c in clips]).astype(np.float32)
    res = {pipe: _first_iteration(rt, plan, d, lengths, clips, wm, pipe) for pipe in ("f16x2", "f32")}
    batch, g4, l4, p4 = res["f16x2"]
    _, g0, l0, p0 = res["f32"]
    assert bool(torch.isfinite(g4).all()) and np.isfinite(l4).all()
    rel = np.asarray([((g4[a:b] - g0[a:b]).norm() / g0[a:b].norm()).item()
                      for a, b in zip(batch.frame_offsets[:-1], batch.frame_offsets[1:])])
    print(f"f16x2 vs f32, last channel group dominant: loss {np.abs(l4 - l0).max():.1e} pred {np.abs(p4 - p0).max():.1e} "
          f"gradient rel L2 median {np.median(rel):.1e} max {rel.max():.1e}")
    assert np.abs(l4 - l0).max() < 1e-5 and np.abs(p4 - p0).max() < 1e-5
    assert rel.max() < 2e-2, rel
