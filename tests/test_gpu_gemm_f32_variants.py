"""Every tile configuration of the f32-MFMA GEMM and the guarded / odd-K-tile forms of the clip-aligned GEMM, alone, against
integer arithmetic (exact) and fp64 (csrc/detector_kernels.hip).

tests/test_gemm_f32_variants_host.py proves that SHAPES and the clip lists below reach every loader pass, K-tail, pipeline
depth, edge tile and tile order of every configuration; change the lists there and here together.

Random operands are seeded per shape: `gemm_seed` for the plain GEMM, `clip_seed` for the clip kernel's normalising
epilogues.  clip_seed is B * 1000 + Tp + N + K + epi, as test_gemm_clip_x3 seeds its inputs, except for the cases listed
in CLIP_SEEDS.  The rule: on a case's inputs the float32 evaluation of the block must stay within half of the test's bars of
the float64 one (a column whose variance over a short clip is near the 1e-5 epsilon does not: no f32 kernel could meet the bar
there, and a column whose bias dwarfs its four-term products loses the digits in z - mean); a default seed that breaks the
rule is replaced by the default plus the first multiple of 1 000 003 that keeps it.  The host module checks the rule for every
case.  Replaced, as (N, K, B, Tp, epi): seed -- (132, 4, 3, 31, 1): 2003174, (132, 4, 3, 128, 1): 1003268,
(132, 4, 8, 5, 1): 2008148, (132, 4, 8, 33, 1): 1008173, (260, 68, 8, 5, 1): 2008340, (128, 160, 3, 5, 1): 1003297,
(128, 96, 3, 5, 1): 1003233, (128, 96, 3, 5, 2): 1003234; every other case runs its default."""
import pytest
import torch

from test_gpu_kernels import _block_reference

pytestmark = pytest.mark.gpu

VARIANTS = list(range(1, 17))
# (M, N, K) of the plain GEMM
SHAPES = [(1, 1, 4), (3, 5, 8), (130, 72, 4), (97, 72, 36), (130, 132, 68), (200, 260, 132), (64, 64, 200), (192, 128, 256),
          (384, 256, 96), (760, 500, 36), (64, 40, 6016), (66, 36, 20), (40, 200, 260)]
SENTINEL = -7777.25                  # no sum of integers, and no plausible sum of the random operands

# the clip-aligned kernel: (N, K), clips per batch, rows per clip of the plain and of the normalising epilogues
CLIP_NK = [(132, 36), (40, 132), (132, 4), (260, 68), (128, 160), (128, 96), (200, 128)]
CLIP_B = [3, 8]
CLIP_TP_EXACT = [1, 2, 31, 33, 64, 65, 96, 97, 128]
CLIP_TP_NORM = [5, 31, 33, 64, 65, 96, 97, 128]
# (N, K, B, Tp, epi) -> seed, where the default does not satisfy the rule of the docstring
CLIP_SEEDS = {(132, 4, 3, 31, 1): 2003174, (132, 4, 3, 128, 1): 1003268, (132, 4, 8, 5, 1): 2008148, (132, 4, 8, 33, 1): 1008173,
              (260, 68, 8, 5, 1): 2008340, (128, 160, 3, 5, 1): 1003297, (128, 96, 3, 5, 1): 1003233,
              (128, 96, 3, 5, 2): 1003234}


def gemm_seed(M, N, K):
    return M * 1000003 + N * 1009 + K


def clip_seed(N, K, B, Tp, epi):
    return CLIP_SEEDS.get((N, K, B, Tp, epi), B * 1000 + Tp + N + K + epi)


def clip_inputs(N, K, B, Tp, epi):
    """The operands of test_gemm_clip_x3 at this case's seed: (a, w, bias, act, rstd), on the host."""
    RP = 32 * ((Tp + 31) // 32)
    g = torch.Generator().manual_seed(clip_seed(N, K, B, Tp, epi))
    a = torch.randn(B * RP, K, generator=g)
    a.view(B, RP, K)[:, Tp:] = 0
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-6, 4, (N, 1), generator=g).float()) / K ** 0.5
    bias = torch.randn(N, generator=g) * 0.1 if epi != 2 else None
    act = torch.randn(B * RP, N, generator=g) if epi == 2 else None
    rstd = torch.rand(B, N, generator=g) + 0.5 if epi == 2 else None
    return a, w, bias, act, rstd


@pytest.fixture(scope="module")
def rt():
    from aware_amd import runtime
    from aware_amd._lib import require_gpu
    require_gpu()
    return runtime


def _integers(shape, g):
    return torch.randint(-8, 9, shape, generator=g).float()


def _pitched(t, pitch):
    """A device copy of t as a view of a [rows + 2, pitch] buffer whose every other element is NaN: a load outside the view
    poisons the result."""
    buf = torch.full((t.shape[0] + 2, pitch), float("nan"), device="cuda")
    buf[:t.shape[0], :t.shape[1]] = t.cuda()
    return buf[:t.shape[0], :t.shape[1]]


class _Case:
    """One shape's operands on the host and the device, its references, and variant 4's outputs: built once, never changed."""

    def __init__(self, rt, M, N, K):
        g = torch.Generator().manual_seed(gemm_seed(M, N, K))
        self.host = {"int": (_integers((M, K), g), _integers((N, K), g), _integers((N,), g)),
                     "float": (torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g))}
        ai, bi, ci = self.host["int"]
        prod = ai.long() @ bi.long().T
        assert int(prod.abs().max()) + 8 < 2 ** 24
        af, bf, cf = self.host["float"]
        prod64 = af.double() @ bf.double().T
        # [kind][with bias]
        self.ref = {"int": {False: prod.double(), True: (prod + ci.long()).double()},
                    "float": {False: prod64, True: prod64 + cf.double()}}
        self.dev = {}
        for kind, (a, b, c) in self.host.items():
            self.dev[kind, False] = (a.cuda(), b.cuda(), c.cuda())
            self.dev[kind, True] = (_pitched(a, K + 4), _pitched(b, K + 8), c.cuda())
        a, b, c = self.dev["float", False]
        self.base = {wb: rt.gemm_nt_variant(a, b, c if wb else None, 4).cpu() for wb in (False, True)}


_cases = {}


def _case(rt, M, N, K):
    if (M, N, K) not in _cases:
        _cases[M, N, K] = _Case(rt, M, N, K)
    return _cases[M, N, K]


def _run(rt, case, kind, with_bias, pitched, variant, M, N):
    """One launch; returns the [M, N] result on the host after checking that nothing else of the buffer was written."""
    a, b, c = case.dev[kind, pitched]
    bias = c if with_bias else None
    if not pitched:
        out = rt.gemm_nt_variant(a, b, bias, variant)
        assert out.shape == (M, N) and out.is_contiguous()
        return out.cpu()
    buf = torch.full((M + 2, N + 3), SENTINEL, device="cuda")
    out = rt.gemm_nt_variant(a, b, bias, variant, out=buf[:M, :N])
    assert out.data_ptr() == buf.data_ptr() and out.stride(0) == N + 3
    full = buf.cpu()
    assert torch.all(full[:M, N:] == SENTINEL) and torch.all(full[M:] == SENTINEL), "wrote outside the [M, N] view"
    return full[:M, :N].clone()


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_gemm_nt_variant(rt, variant, M, N, K):
    """Exact on integer operands, within test_gemm_nt's bar of fp64 on random ones, bit-identical to variant 4, and nothing
    written outside C: with and without bias, contiguous and row-pitched (lda = K + 4, ldb = K + 8, ldc = N + 3)."""
    case = _case(rt, M, N, K)
    worst = 0.0
    for with_bias in (True, False):
        for pitched in (False, True):
            what = (variant, (M, N, K), "bias" if with_bias else "no bias", "pitched" if pitched else "contiguous")
            out = _run(rt, case, "int", with_bias, pitched, variant, M, N)
            wrong = (out.double() != case.ref["int"][with_bias]).nonzero()
            assert wrong.numel() == 0, (what, "first wrong elements (row, col):", wrong[:8].tolist())
            out = _run(rt, case, "float", with_bias, pitched, variant, M, N)
            ref = case.ref["float"][with_bias]
            # the bar of test_gemm_nt, on the scale of the biased product as there
            scale = case.ref["float"][True].abs().max().item()
            err = (out.double() - ref).abs().max().item()
            worst = max(worst, err / scale)
            assert err < 2e-6 * scale * max(1.0, K / 256), (what, err, scale)
            assert torch.equal(out, case.base[with_bias]), (what, "differs from variant 4 in",
                                                            int((out != case.base[with_bias]).sum()), "elements")
    print(f"variant {variant} {M}x{N}x{K}: worst error / max|ref| {worst:.2e} (bar {2e-6 * max(1.0, K / 256):.1e})")


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_automatic_choice_matches_variant_4(rt, M, N, K):
    """Variant 0, and gemm_nt which runs it, whatever the process has tuned so far."""
    case = _case(rt, M, N, K)
    a, b, c = case.dev["float", False]
    for with_bias in (True, False):
        bias = c if with_bias else None
        assert torch.equal(rt.gemm_nt_variant(a, b, bias, 0).cpu(), case.base[with_bias])
        assert torch.equal(rt.gemm_nt(a, b, bias).cpu(), case.base[with_bias])


@pytest.mark.parametrize("variant", [17, -1])
def test_unknown_variant_is_refused(rt, variant):
    import ctypes as C
    from aware_amd._lib import AwareHipError, load_library
    a, b = torch.ones(8, 8, device="cuda"), torch.ones(8, 8, device="cuda")
    out = torch.full((8, 8), SENTINEL, device="cuda")
    rc = load_library().aware_gemm_nt_variant(C.c_void_p(a.data_ptr()), 8, C.c_void_p(b.data_ptr()), 8, None,
                                              C.c_void_p(out.data_ptr()), 8, 8, 8, 8, variant,
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -1                                         # AWARE_E_BADARG
    with pytest.raises(AwareHipError, match="bad argument"):
        rt.gemm_nt_variant(a, b, None, variant, out=out)
    assert torch.all(out.cpu() == SENTINEL)


def test_wrapper_refuses_what_the_kernel_cannot_address(rt):
    a, b = torch.ones(8, 8, device="cuda"), torch.ones(8, 8, device="cuda")
    with pytest.raises(ValueError):
        rt.gemm_nt_variant(a.T, b, None, 4)                                        # column stride
    with pytest.raises(ValueError):
        rt.gemm_nt_variant(a, b[:, :4], None, 4)                                   # K differs
    with pytest.raises(ValueError):
        rt.gemm_nt_variant(a, b, None, 4, out=torch.empty(8, 9, device="cuda"))    # shape of out
    with pytest.raises(ValueError):
        rt.gemm_nt_variant(a, b, torch.ones(7, device="cuda"), 4)                  # bias length


# ---------------------------------------------------------------------------------------------
# gemm_clip_kernel through rt.gemm_clip(..., mode=0)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tp", CLIP_TP_EXACT)
@pytest.mark.parametrize("B", CLIP_B)
@pytest.mark.parametrize("N,K", CLIP_NK)
def test_gemm_clip_plain_is_exact_on_integers(rt, N, K, B, Tp):
    """epi 0 on integers in [-8, 8]: rows below Tp equal the integer product plus bias exactly, the rows up to the 32-row
    boundary are written as zero although A's rows there are not."""
    RP = 32 * ((Tp + 31) // 32)
    g = torch.Generator().manual_seed(gemm_seed(B * RP, N, K) + Tp)
    a, w, bias = _integers((B * RP, K), g), _integers((N, K), g), _integers((N,), g)
    ref = (a.long() @ w.long().T + bias.long()).view(B, RP, N)
    for bv in (bias, None):
        c, _ = rt.gemm_clip(a.cuda(), w.cuda(), None if bv is None else bv.cuda(), B, Tp, 0, mode=0)
        c = c.cpu().view(B, RP, N)
        want = (ref if bv is not None else ref - bias.long())[:, :Tp].double()
        wrong = (c[:, :Tp].double() != want).nonzero()
        assert wrong.numel() == 0, ("first wrong elements (clip, row, col):", wrong[:8].tolist())
        assert RP == Tp or c[:, Tp:].abs().max().item() == 0.0


@pytest.mark.parametrize("Tp", CLIP_TP_NORM)
@pytest.mark.parametrize("epi", [1, 2])
@pytest.mark.parametrize("B", CLIP_B)
@pytest.mark.parametrize("N,K", CLIP_NK)
def test_gemm_clip_norm_epilogues(rt, N, K, B, epi, Tp):
    """epi 1 (InstanceNorm + LeakyReLU) and epi 2 (their backward) against fp64 at the bars of test_gemm_clip_x3."""
    RP = 32 * ((Tp + 31) // 32)
    a, w, bias, act, rstd = clip_inputs(N, K, B, Tp, epi)
    ref = _block_reference(a, w, bias, act, rstd, B, RP, Tp, epi)
    c, rs = rt.gemm_clip(a.cuda(), w.cuda(), None if bias is None else bias.cuda(), B, Tp, epi,
                         None if rstd is None else rstd.cuda(), None if act is None else act.cuda(), 0)
    c = c.cpu().view(B, RP, N)
    assert RP == Tp or c[:, Tp:].abs().max().item() == 0.0
    ers = 0.0
    if epi == 1:
        z = (a.double() @ w.double().T).view(B, RP, N)[:, :Tp] + bias.double()
        ref_rs = 1.0 / torch.sqrt(z.var(1, unbiased=False) + 1e-5)
        ers = ((rs.cpu().double() - ref_rs).abs() / ref_rs).max().item()
    scale = ref.abs().amax(dim=(0, 1), keepdim=True).clamp_min(1e-30)
    err = ((c[:, :Tp].double() - ref).abs() / scale).max().item()
    print(f"clip N={N} K={K} B={B} Tp={Tp} epi={epi}: column-relative error {err:.2e}, rstd relative error {ers:.2e}")
    assert err < 4e-6 * max(1.0, K / 256), err
    assert ers < 2e-5, ers
