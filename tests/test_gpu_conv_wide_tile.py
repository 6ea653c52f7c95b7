"""The wide form of the f16 two-term conv kernel (gemm_h2.hip: 4 waves x 64 columns per workgroup, 256-column slabs) against
its 128-column form (8 waves x 16 columns): the same bits in every output, at the GEMM and through the embed loop, and the
rule by which a session's plan chooses between them.

Run on the MI355X box:  python -m pytest tests/test_gpu_conv_wide_tile.py -m gpu -q -s
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPIS = ("plain", "forward", "backward", "forward_last")
CL = 40


@pytest.fixture(scope="module")
def rt():
    from aware_amd import runtime
    from aware_amd._lib import require_gpu
    require_gpu()
    return runtime


@pytest.fixture(scope="module")
def plan(rt):
    return rt.Plan()


@pytest.fixture(scope="module")
def det(rt, plan):
    from oracle import aware_oracle as O
    ws, bs = O.detector_weights()
    return rt.DetectorWeights(plan, O.mel_filter_bank(), [w.numpy() for w in ws], [b.numpy() for b in bs])


def _operands(B, Tp, N, K, seed):
    """Seeded normal A (zero padding rows), weights spanning 2^10 per row (as test_gemm_clip_h2_wide_dynamic_range), and the
    extra operands of the epilogues."""
    RP = 32 * ((Tp + 31) // 32)
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, RP, K, generator=g)
    a[:, Tp:] = 0
    w = torch.randn(N, K, generator=g) * torch.exp2(-20 * torch.rand(N, K, generator=g) ** 4)
    w = w * torch.exp2(torch.randint(-10, 4, (N, 1), generator=g).float()) / K ** 0.5
    bias = torch.randn(N, generator=g) * 0.1
    act = torch.randn(B, RP, N, generator=g)
    act[:, Tp:] = 0
    rstd = torch.rand(B, N, generator=g) + 0.5
    wl = torch.randn(CL, N, generator=g) * torch.exp2(torch.randint(-4, 3, (CL, 1), generator=g).float()) / N ** 0.5
    return a, w, bias, act.reshape(B * RP, N), rstd, wl


def _run(rt, a, w, bias, act, rstd, wl, B, Tp, epi, tile):
    """(C, rstd, amax partials[, zpart]) of one epilogue on one form of the kernel"""
    K = a.shape[-1]
    ad, wd = a.reshape(-1, K).cuda(), w.cuda()
    if epi == "plain":
        return rt.gemm_clip_h2(ad, wd, bias.cuda(), B, Tp, 0, tile=tile)
    if epi == "forward":
        return rt.gemm_clip_h2(ad, wd, bias.cuda(), B, Tp, 1, tile=tile)
    if epi == "backward":
        return rt.gemm_clip_h2(ad, wd, None, B, Tp, 2, rstd.cuda(), act.cuda(), tile=tile)
    return rt.gemm_clip_h2(ad, wd, bias.cuda(), B, Tp, 1, w_last=wl, tile=tile)


def _same_bits(rt, ops, B, Tp, N, what):
    for epi in EPIS:
        narrow = _run(rt, *ops, B, Tp, epi, 1)
        wide = _run(rt, *ops, B, Tp, epi, 2)
        names = ("C", "rstd", "amax", "zpart")
        assert len(narrow) == len(wide) == (4 if epi == "forward_last" else 3)
        for name, x, y in zip(names, narrow, wide):
            if name == "amax":
                x, y = x[:, :N // 16], y[:, :N // 16]
            assert bool(torch.isfinite(x).all()), (what, epi, name)
            assert torch.equal(x, y), (what, epi, name, int((x != y).sum()), float((x - y).abs().max()))
        # something was computed: the outputs are not all zero where the operands are not
        if float(ops[0].abs().max()) > 0 and epi != "backward":
            assert float(wide[0].abs().max()) > 0, (what, epi)


@pytest.mark.parametrize("N,K", [(256, 64), (512, 128), (1024, 512), (512, 1024), (1024, 1024)])
@pytest.mark.parametrize("Tp", [17, 47, 94])
@pytest.mark.parametrize("B", [3, 8, 16])
def test_both_forms_same_bits(rt, B, Tp, N, K):
    """C, rstd, the amax partials and (last-block epilogue, CL = 40) zpart of the wide form equal those of the 128-column form
    bit for bit: plain, forward, backward and forward-with-last-block epilogues; B = 3 takes the plain block walk, 8 and 16
    the XCD walk with one and two clips per XCD; Tp = 17, 47, 94 give one, two and three 32-row groups, each with padding
    rows; the shapes give one and several tiles per clip, one K tile and many, and (1024 x 1024: 3 of 4 tiles fit, so groups
    of 2) a slab-group size below the tile count."""
    ops = _operands(B, Tp, N, K, 1000 * B + 10 * Tp + N + K)
    _same_bits(rt, ops, B, Tp, N, (B, Tp, N, K))


@pytest.mark.parametrize("Tp,N,K", [(94, 1024, 512), (47, 512, 128)])
def test_both_forms_same_bits_per_clip_scales(rt, Tp, N, K):
    """One clip of a batch of 8 scaled by 2^-30, one by 2^+20 (per-clip operand scales) and one all-zero clip."""
    B = 8
    a, w, bias, act, rstd, wl = _operands(B, Tp, N, K, 77 + Tp)
    a[2] *= 2.0 ** -30
    a[5] *= 2.0 ** 20
    a[6] = 0
    _same_bits(rt, (a, w, bias, act, rstd, wl), B, Tp, N, ("scales", Tp, N, K))


@pytest.mark.parametrize("B,Tp,N,K", [(8, 100, 512, 128), (8, 47, 128, 128)])
def test_unsupported_shapes(rt, B, Tp, N, K):
    """Four 32-row groups per clip (Tp = 100) and N = 128: the wide form refuses (AWARE_E_UNSUPPORTED), tile 0 gives the
    128-column form's bits."""
    from aware_amd._lib import AwareHipError
    ops = _operands(B, Tp, N, K, 5 + Tp + N)
    for epi in ("plain", "forward", "backward"):
        with pytest.raises(AwareHipError, match="unsupported"):
            _run(rt, *ops, B, Tp, epi, 2)
        for x, y in zip(_run(rt, *ops, B, Tp, epi, 0), _run(rt, *ops, B, Tp, epi, 1)):
            assert torch.equal(x, y), (epi, Tp, N)


def _loop(rt, plan, det, B, conv_tile, iters=20):
    n = 16000
    batch = rt.Batch([n] * B)
    g = torch.Generator().manual_seed(11)
    audio = (0.1 * torch.randn(B * n, generator=g)).cuda()
    target = (torch.randint(0, 2, (B, det.n_bits), generator=g).float() * 2 - 1).cuda()
    sess = rt.EmbedSession(plan, det, batch, use_graph=True, conv_tile=conv_tile, num_iterations=iters)
    sess.begin(audio, target)
    losses = []
    for _ in range(iters):
        sess.iterate(1)
        losses.append(sess.loss.clone())
    torch.cuda.synchronize()
    out = dict(coef=sess.coef.clone(), best=sess.best_coef.clone(), best_loss=sess.best_loss.clone(), pred=sess.pred.clone(),
               losses=torch.stack(losses))
    return out, sess.conv_tiles()


# the smallest batch of 1 s clips for which the automatic rule takes the wide form on the 1024-channel launches:
# (1024 / 256) * B >= 512 workgroups (32 clips give 128, below the rule's threshold)
LOOP_CLIPS = 128


def test_loop_same_bits(rt, plan, det):
    """20 iterations through the graph path on 128 clips of 1 s with the 128-column form and with the wide form: coefficients,
    best snapshot, losses and detected values equal bit for bit; the wide session runs the wide form on every f16 two-term
    conv launch (all of them support it: 31 pooled rows, N = 512 or 1024), and the automatic rule picks it for this batch."""
    narrow, tn = _loop(rt, plan, det, LOOP_CLIPS, "narrow")
    wide, tw = _loop(rt, plan, det, LOOP_CLIPS, "wide")
    auto, ta = _loop(rt, plan, det, LOOP_CLIPS, "auto")
    print("conv tiles (forward, backward): narrow", tn, "wide", tw, "auto", ta)
    assert 2 not in tn[0] + tn[1] and 1 in tn[0] and 1 in tn[1]
    assert [t == 2 for t in tw[0]] == [t == 1 for t in tn[0]] and [t == 2 for t in tw[1]] == [t == 1 for t in tn[1]]
    assert 2 in ta[0] + ta[1]
    for k in narrow:
        assert bool(torch.isfinite(narrow[k]).all())
        assert torch.equal(narrow[k], wide[k]), (k, int((narrow[k] != wide[k]).sum()))
        assert torch.equal(narrow[k], auto[k]), (k, int((narrow[k] != auto[k]).sum()))
    assert float(narrow["losses"][-1].mean()) < float(narrow["losses"][0].mean())


def test_selection_rule_small_batch(rt, plan, det):
    """The automatic rule on grids too small for the wide form: 8 clips (below the f16 two-term kernel's own grid threshold)
    and 32 clips (the f16 kernel runs; its wide form would have 64 or 128 workgroups) report no wide launch, and the 32-clip
    session reports the 128-column form on every f16 two-term launch."""
    for B in (8, 32):
        sess = rt.EmbedSession(plan, det, rt.Batch([16000] * B), num_iterations=4)
        fwd, bwd = sess.conv_tiles()
        print(B, "clips, automatic: conv tiles", fwd, bwd)
        assert 2 not in fwd + bwd
        if B == 32:
            assert 1 in fwd and 1 in bwd
