"""The row-major epilogue of the wide f16 two-term conv kernel (conv_block.hpp, ROWS: C stores and the data gradient's act
loads as whole 128-byte row pieces through a wave-private LDS region) against the 128-column form, bit for bit, where
tests/test_gpu_conv_wide_tile.py cannot see: clips without padding rows, the zeros of the padding rows, writes outside the
tile, the accumulator-layout epilogue that unaligned buffers fall back to, and the last-block epilogue at several CL.

Every run writes into the caller's buffer: [M + 32 rows][ldc] filled with a canary, the [M][N] view of C pre-filled with NaN.

Run on the MI355X box:  python -m pytest tests/test_gpu_conv_epilogue_rows.py -m gpu -q -s
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPIS = ("plain", "forward", "backward", "forward_last")
CANARY = -12345.678
TAIL = 32                       # canary rows past the last clip


@pytest.fixture(scope="module")
def rt():
    from aware_amd import runtime
    from aware_amd._lib import require_gpu
    require_gpu()
    return runtime


def _operands(B, Tp, N, K, CL, seed):
    """Seeded normal A and act (zero padding rows), weights spanning 2^10 per row, as tests/test_gpu_conv_wide_tile.py"""
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
    return dict(a=a.reshape(B * RP, K).cuda(), w=w.cuda(), bias=bias.cuda(), act=act.reshape(B * RP, N).cuda(), rstd=rstd.cuda(),
                wl=wl, B=B, Tp=Tp, N=N, K=K, RP=RP)


def _run(rt, ops, epi, tile, pad, want_form):
    """One epilogue on one form into a canary-framed buffer of row pitch N + pad.  Checks the frame, the padding rows and the
    form the launcher reports; returns (C, rstd, amax[:, :N/16][, zpart])."""
    B, Tp, N, K, RP = ops["B"], ops["Tp"], ops["N"], ops["K"], ops["RP"]
    M, ldc = B * RP, N + pad
    buf = torch.full((M + TAIL, ldc), CANARY, device="cuda")
    c = buf[:M, :N]
    c.fill_(float("nan"))
    act = None
    if epi == "backward":
        abuf = torch.full((M + TAIL, ldc), CANARY, device="cuda")
        act = abuf[:M, :N]
        act.copy_(ops["act"])
    code = {"plain": 0, "forward": 1, "backward": 2, "forward_last": 1}[epi]
    last = epi == "forward_last"
    assert rt.gemm_clip_h2_form(c, act, Tp, K, code, last, tile) == want_form, (epi, tile, pad)
    res = rt.gemm_clip_h2(ops["a"], ops["w"], None if epi == "backward" else ops["bias"], B, Tp, code,
                          ops["rstd"].clone() if epi == "backward" else None, act, w_last=ops["wl"] if last else None, tile=tile,
                          out=c)
    what = (epi, tile, pad, B, Tp, N, K)
    assert res[0].data_ptr() == c.data_ptr()
    # no stray writes: the gap columns and the rows past the last clip still hold the canary
    frame = torch.full_like(buf, CANARY)
    assert torch.equal(buf[:M, N:], frame[:M, N:]) and torch.equal(buf[M:], frame[M:]), what
    if act is not None:
        assert torch.equal(abuf[:M, N:], frame[:M, N:]) and torch.equal(abuf[M:], frame[M:]) and torch.equal(act, ops["act"]), what
    # every element was written; the padding rows of every clip are exactly +0.0
    assert not bool(torch.isnan(c).any()), what
    padrows = c.reshape(B, RP, N)[:, Tp:]
    assert bool((padrows == 0).all()) and not bool(torch.signbit(padrows).any()), what
    out = [c.clone(), res[1], res[2][:, :N // 16]]
    if last:
        out.append(res[3])
    return out


def _same_bits(rt, ops, epis=EPIS, pad=4, wide_form=3):
    for epi in epis:
        narrow = _run(rt, ops, epi, 1, pad, 1)
        wide = _run(rt, ops, epi, 2, pad, wide_form)
        assert len(narrow) == len(wide) == (4 if epi == "forward_last" else 3)
        for name, x, y in zip(("C", "rstd", "amax", "zpart"), narrow, wide):
            what = (epi, name, pad, ops["B"], ops["Tp"], ops["N"], ops["K"])
            assert bool(torch.isfinite(x).all()), what
            assert torch.equal(x, y), what + (int((x != y).sum()), float((x - y).abs().max()))
        # something was computed (a single row normalises to zero; the data gradient of unrelated operands may be anything)
        if epi == "plain" or (epi != "backward" and ops["Tp"] > 1):
            assert float(wide[0].abs().max()) > 0, (epi, "all zero")


@pytest.mark.parametrize("N,K", [(256, 64), (512, 128)])
@pytest.mark.parametrize("Tp", [1, 16, 17, 32, 33, 64, 65, 95, 96])
@pytest.mark.parametrize("B", [1, 8])
def test_row_group_edges(rt, B, Tp, N, K):
    """Wide (row-major epilogue) against 128-column on C, rstd, amax and zpart at the edges of the 32-row groups: Tp = 32, 64
    and 96 have no padding row, 1 / 33 / 65 a single valid row in the last group; one clip (plain walk) and eight (XCD walk);
    one and two wide slabs per clip.  ldc = N + 4: the four gap columns and 32 rows past the last clip keep their canary, the
    padding rows come out as +0.0 over the NaN pre-fill."""
    _same_bits(rt, _operands(B, Tp, N, K, 40, 7 * B + 100 * Tp + N + K))


@pytest.mark.parametrize("Tp", [17, 96])
def test_contiguous_rows(rt, Tp):
    """ldc = N, the pitch of the embed loop: the same comparison without gap columns"""
    _same_bits(rt, _operands(8, Tp, 512, 128, 40, 3 + Tp), pad=0)


@pytest.mark.parametrize("pad", [1, 2, 3])
@pytest.mark.parametrize("Tp", [17, 64, 96])
def test_unaligned_pitch_takes_the_accumulator_layout(rt, Tp, pad):
    """ldc = N + 1 (and + 2, + 3): the launcher reports the wide form's accumulator-layout epilogue (form 2) and the results
    equal the 128-column form bit for bit; the aligned launches above report the row-major one (form 3)."""
    _same_bits(rt, _operands(8, Tp, 512, 128, 40, 11 + Tp + pad), pad=pad, wide_form=2)


@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("Tp", [17, 96])
@pytest.mark.parametrize("CL", [1, 17, 40, 48])
def test_forward_last(rt, CL, Tp, N):
    """The last-block epilogue stores C from the f32 slab it lays out for the split-K partials: one, two and three column
    tiles of the last conv (CL = 1 and 17: partial tiles), one and two 128-column slabs per wave pair."""
    _same_bits(rt, _operands(8, Tp, N, 128, CL, 5 * CL + Tp + N), epis=("forward_last",))
