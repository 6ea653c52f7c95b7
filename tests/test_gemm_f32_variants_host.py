"""The tile table of the f32-MFMA GEMM (gemm_dispatch, csrc/detector_kernels.hip) restated, and the proof that the shape lists of
tests/test_gpu_gemm_f32_variants.py drive every one of its 16 configurations, and the clip-aligned kernel, through each path
on which a configuration can be wrong on its own (no device)."""
import os
import re

import pytest
import torch

from test_gpu_gemm_f32_variants import CLIP_B, CLIP_NK, CLIP_TP_EXACT, CLIP_TP_NORM, SHAPES, clip_inputs, clip_seed
from test_gpu_kernels import _block_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# variant: (BM, BN, NWM, NWN, BK, DB) -- block tile, waves along M and N, K tile, LDS buffers
TILES = {1: (128, 128, 2, 2, 32, 1), 2: (128, 64, 2, 2, 32, 1), 3: (64, 64, 2, 2, 32, 2), 4: (64, 64, 2, 2, 32, 1),
         5: (64, 64, 2, 2, 16, 2), 6: (64, 64, 2, 2, 64, 1), 7: (64, 128, 2, 2, 32, 1), 8: (128, 128, 4, 2, 16, 2),
         9: (96, 64, 3, 2, 32, 1), 10: (128, 64, 4, 2, 32, 1), 11: (64, 128, 2, 4, 32, 1), 12: (128, 128, 4, 4, 32, 1),
         13: (96, 128, 3, 4, 32, 1), 14: (96, 128, 3, 4, 16, 2), 15: (96, 64, 3, 2, 16, 2), 16: (96, 128, 3, 4, 32, 2)}
NUM_TUNED = 12                       # gemm_autotune times variants 1..NUM_TUNED
HEURISTIC = {4, 5, 6, 10}            # what gemm_heuristic may return
CLIP_BN, CLIP_BK = 128, 32           # gemm_clip_kernel as launch_gemm_clip instantiates it: NWN = 4, BK = 32, one buffer


def _source():
    return open(os.path.join(ROOT, "aware_amd", "csrc", "detector_kernels.hip")).read()


def test_table_matches_the_source():
    src = _source()
    body = src[src.index("static void gemm_dispatch("):src.index("#undef GL")]
    cases = {int(m.group(1)): tuple(int(x) for x in m.group(2).split(","))
             for m in re.finditer(r"case (\d+): GL\(([\d, ]+)\); break;", body)}
    assert cases == TILES
    assert tuple(int(x) for x in re.search(r"default: GL\(([\d, ]+)\); break;", body).group(1).split(",")) == TILES[4]
    assert int(re.search(r"constexpr int kNumGemmVariants = (\d+);", src).group(1)) == NUM_TUNED
    heur = src[src.index("static int gemm_heuristic("):src.index("static int gemm_lookup(")]
    plain = re.findall(r"return (\d+);", heur)
    either = re.findall(r"return \([^;?]*\) \? (\d+) : (\d+);", heur)
    assert len(plain) == 2 and len(either) == 1 and heur.count("return") == 3
    assert {int(x) for x in plain} | {int(x) for x in either[0]} == HEURISTIC
    # the entry point serves exactly the table's rows and 0
    capi = open(os.path.join(ROOT, "aware_amd", "csrc", "capi.hip")).read()
    entry = capi[capi.index('extern "C" int aware_gemm_nt_variant('):]
    assert f"variant < 0 || variant > {max(TILES)})" in entry[:entry.index("}")]
    clip = src[src.index("void launch_gemm_clip("):src.index("#undef CLE")]
    assert "clip_launch<M_, 4, E_, K_, D_>" in clip and f"CLE({CLIP_BK}, 1)" in clip


@pytest.mark.parametrize("variant", sorted(TILES))
def test_tiles_are_buildable(variant):
    """What the kernel's static_assert and the device demand of a row: whole 32x32 MFMA tiles per wave, whole k-groups of 8
    per K tile, at most 1024 threads and 64 KiB of LDS."""
    BM, BN, NWM, NWN, BK, DB = TILES[variant]
    assert BM % (32 * NWM) == 0 and BN % (32 * NWN) == 0 and BK % 8 == 0 and DB in (1, 2)
    assert 64 * NWM * NWN <= 1024 and (64 * NWM * NWN) % (BK // 4) == 0
    assert DB * (BM + BN) * (BK + 4) * 4 <= 65536


def _grid(variant, M, N, K):
    BM, BN, _, _, BK, _ = TILES[variant]
    tm, tn = -(-M // BM), -(-N // BN)
    return BM, BN, BK, tm, tn, tm * tn, -(-K // BK)


def _partial(variant, M, N):
    BM, BN = TILES[variant][:2]
    return M % BM != 0 or N % BN != 0


# property name -> predicate(variant, M, N, K)
GEMM_PROPERTIES = {
    "nk = 1": lambda v, M, N, K: _grid(v, M, N, K)[6] == 1,
    "nk = 2": lambda v, M, N, K: _grid(v, M, N, K)[6] == 2,
    "nk = 3": lambda v, M, N, K: _grid(v, M, N, K)[6] == 3,
    "nk even, >= 4": lambda v, M, N, K: _grid(v, M, N, K)[6] >= 4 and _grid(v, M, N, K)[6] % 2 == 0,
    "nk odd, >= 5": lambda v, M, N, K: _grid(v, M, N, K)[6] >= 5 and _grid(v, M, N, K)[6] % 2 == 1,
    "K % BK != 0": lambda v, M, N, K: K % TILES[v][4] != 0,
    "K % 8 == 4": lambda v, M, N, K: K % 8 == 4,
    "M % BM != 0, several tile rows": lambda v, M, N, K: M % TILES[v][0] != 0 and _grid(v, M, N, K)[3] > 1,
    "M < BM": lambda v, M, N, K: M < TILES[v][0],
    "N % BN != 0, several tile columns": lambda v, M, N, K: N % TILES[v][1] != 0 and _grid(v, M, N, K)[4] > 1,
    "N < 32": lambda v, M, N, K: N < 32,
    "swizzled grid with partial tiles": lambda v, M, N, K: (_grid(v, M, N, K)[5] > 1 and _grid(v, M, N, K)[5] % 8 == 0
                                                            and _partial(v, M, N)),
    "grid of several tiles, not swizzled": lambda v, M, N, K: _grid(v, M, N, K)[5] > 1 and _grid(v, M, N, K)[5] % 8 != 0,
    "every tile full": lambda v, M, N, K: not _partial(v, M, N),
}


@pytest.mark.parametrize("name", sorted(GEMM_PROPERTIES))
def test_every_variant_meets(name):
    pred = GEMM_PROPERTIES[name]
    missing = [v for v in sorted(TILES) if not any(pred(v, *s) for s in SHAPES)]
    assert not missing, f"no shape of SHAPES gives variants {missing}: {name}"


def test_shapes_are_legal_and_exact_on_integers():
    """What the ABI demands (K a multiple of 4, at least 4) and what check 1 of the device test rests on: with operands and
    bias in [-8, 8] every partial sum is an integer of magnitude at most 64 K + 8 < 2^24, so f32 holds it exactly."""
    assert len(set(SHAPES)) == len(SHAPES)
    for M, N, K in SHAPES:
        assert M >= 1 and N >= 1 and K >= 4 and K % 4 == 0
        assert 64 * K + 8 < 2 ** 24
    for N, K in CLIP_NK:
        assert K >= 4 and K % 4 == 0 and 64 * K + 8 < 2 ** 24


def _clip_cases():
    return [(B, N, K) for N, K in CLIP_NK for B in CLIP_B]


CLIP_PROPERTIES = {
    **{f"nk = {n}": (lambda B, N, K, n=n: -(-K // CLIP_BK) == n) for n in (1, 2, 3, 4, 5)},
    **{f"EXACT form, nk = {n}": (lambda B, N, K, n=n: K % CLIP_BK == 0 and N % CLIP_BN == 0 and K // CLIP_BK == n) for n in (3, 5)},
    "guarded by k only in the last K tile": lambda B, N, K: K % CLIP_BK != 0,
    "guarded by N alone": lambda B, N, K: K % CLIP_BK == 0 and N % CLIP_BN != 0,
    "partial last column slab": lambda B, N, K: N % CLIP_BN != 0 and N > CLIP_BN,
    "single partial slab": lambda B, N, K: N < CLIP_BN,
    "swizzled grid (tn * B % 8 == 0)": lambda B, N, K: (-(-N // CLIP_BN) * B) % 8 == 0,
    "swizzled grid with a partial slab": lambda B, N, K: (-(-N // CLIP_BN) * B) % 8 == 0 and N % CLIP_BN != 0,
    "grid not swizzled": lambda B, N, K: (-(-N // CLIP_BN) * B) % 8 != 0,
    "grid not swizzled, several slabs": lambda B, N, K: (-(-N // CLIP_BN) * B) % 8 != 0 and N > CLIP_BN,
}


@pytest.mark.parametrize("name", sorted(CLIP_PROPERTIES))
def test_clip_list_meets(name):
    assert any(CLIP_PROPERTIES[name](*c) for c in _clip_cases()), name


def test_clip_row_counts_cover_every_wave_count_and_edge():
    """Tp selects NWM = ceil(Tp / 32) = 1..4 wave rows; each list holds, for every NWM, a Tp that fills the last 32-row group
    or leaves one row in it, and the plain list the smallest clip."""
    for tps in (CLIP_TP_EXACT, CLIP_TP_NORM):
        assert {-(-t // 32) for t in tps} == {1, 2, 3, 4}
        assert all(1 <= t <= 128 for t in tps)
        assert {32 * n + 1 for n in (1, 2, 3)} <= set(tps) and {64, 96, 128} <= set(tps) and 31 in tps
    assert 1 in CLIP_TP_EXACT and 2 in CLIP_TP_EXACT


def _block_f32(a, w, bias, act, rstd, B, RP, Tp, epi):
    """_block_reference (tests/test_gpu_kernels.py) with every operation in float32; for epi 1 also the reciprocal deviation."""
    N = w.shape[0]
    z = (a @ w.T).view(B, RP, N)[:, :Tp]
    if epi == 1:
        z = z + bias
        rs = 1.0 / torch.sqrt(z.var(1, unbiased=False, keepdim=True) + 1e-5)
        u = (z - z.mean(1, keepdim=True)) * rs
        return torch.where(u > 0, u, 0.2 * u), rs[:, 0]
    av = act.view(B, RP, N)[:, :Tp]
    u = torch.where(av > 0, av, av * 5.0)
    du = z * torch.where(av > 0, 1.0, 0.2)
    return rstd[:, None, :] * (du - du.mean(1, keepdim=True) - u * (du * u).mean(1, keepdim=True)), None


def f32_errors(N, K, B, Tp, epi):
    """(column-relative error, rstd relative error) of the float32 evaluation against the float64 one on a case's inputs."""
    RP = 32 * ((Tp + 31) // 32)
    a, w, bias, act, rstd = clip_inputs(N, K, B, Tp, epi)
    ref = _block_reference(a, w, bias, act, rstd, B, RP, Tp, epi)
    got, rs = _block_f32(a, w, bias, act, rstd, B, RP, Tp, epi)
    scale = ref.abs().amax(dim=(0, 1), keepdim=True).clamp_min(1e-30)
    err = ((got.double() - ref).abs() / scale).max().item()
    ers = 0.0
    if epi == 1:
        z = (a.double() @ w.double().T).view(B, RP, N)[:, :Tp] + bias.double()
        ref_rs = 1.0 / torch.sqrt(z.var(1, unbiased=False) + 1e-5)
        ers = ((rs.double() - ref_rs).abs() / ref_rs).max().item()
    return err, ers


@pytest.mark.parametrize("epi", [1, 2])
@pytest.mark.parametrize("N,K", CLIP_NK)
def test_clip_inputs_are_well_conditioned(N, K, epi):
    """The rule of the device module's docstring: float32 arithmetic in the plainest order stays within HALF of the device
    test's bars on every case's inputs, so a kernel that misses a bar is wrong and not unlucky."""
    for B in CLIP_B:
        for Tp in CLIP_TP_NORM:
            err, ers = f32_errors(N, K, B, Tp, epi)
            assert err < 0.5 * 4e-6 * max(1.0, K / 256), (B, Tp, clip_seed(N, K, B, Tp, epi), err)
            assert ers < 0.5 * 2e-5, (B, Tp, clip_seed(N, K, B, Tp, epi), ers)
