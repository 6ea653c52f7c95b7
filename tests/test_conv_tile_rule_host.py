"""Which form of the f16 two-term conv kernel a uniform batch's plan gives each conv launch (no device): the rule of det_plan /
h2_conv_tile (csrc/capi.hip) and the slab-group computation of the uniform block walk (conv_slab_group, csrc/conv_block.hpp)
restated, on the model card's five launch shapes."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (N, K) of the five conv launches of an iteration: forward of blocks 0..2, data gradients of blocks 2 and 1
LAYERS = {"conv0 fwd": (512, 128), "conv1 fwd": (1024, 512), "conv2 fwd": (1024, 1024), "conv2 bwd": (1024, 1024),
          "conv1 bwd": (512, 1024)}
BATCHES = [8, 32, 64, 256]
L2_BUDGET = 3355443            # bytes of packed weights a slab group may hold (3.2 MB of an XCD's 4 MB L2)
WEIGHT_BYTES = 4               # two f16 terms per weight
NARROW, WIDE = 128, 256        # columns of a workgroup's tile
H2_MIN_GRID, WIDE_MIN_GRID = 128, 512


def supported(rg, N, K):
    return 1 <= rg <= 4 and N % 128 == 0 and K % 64 == 0 and K <= 1024


def wide_supported(rg, N, K):
    return supported(rg, N, K) and rg <= 3 and N % WIDE == 0


def conv_tile(conv_tile_cfg, B, rg, N, K):
    """0: the launch does not run on the uniform f16 two-term kernel; 1: its 128-column form; 2: the wide form."""
    if not (supported(rg, N, K) and (N // NARROW) * B >= H2_MIN_GRID):
        return 0
    if conv_tile_cfg == 1 or not wide_supported(rg, N, K):
        return 1
    if conv_tile_cfg == 2:
        return 2
    return 2 if (N // WIDE) * B >= WIDE_MIN_GRID else 1


def slab_group(tiles_n, width, K):
    sg = L2_BUDGET // (width * K * WEIGHT_BYTES)
    sg = max(1, min(sg, tiles_n))
    while tiles_n % sg:
        sg -= 1
    return sg


def test_constants_match_the_sources():
    capi = open(os.path.join(ROOT, "aware_amd", "csrc", "capi.hip")).read()
    kern = open(os.path.join(ROOT, "aware_amd", "csrc", "kernels.h")).read()
    block = open(os.path.join(ROOT, "aware_amd", "csrc", "conv_block.hpp")).read()
    assert int(re.search(r"constexpr int kH2MinGrid = (\d+);", capi).group(1)) == H2_MIN_GRID
    assert int(re.search(r"constexpr int kH2WideMinGrid = (\d+);", capi).group(1)) == WIDE_MIN_GRID
    assert int(re.search(r"constexpr int kH2WideTile = (\d+);", kern).group(1)) == WIDE
    assert f"{L2_BUDGET}u / (unsigned)(width * K * weight_bytes)" in block
    assert "return (N / kH2WideTile) * B >= kH2WideMinGrid ? 2 : 1;" in capi


@pytest.mark.parametrize("rg", [1, 2, 3, 4])
@pytest.mark.parametrize("B", BATCHES)
def test_rule_on_the_card_shapes(B, rg):
    """Automatic choice: the wide form exactly where it is supported and its grid has >= 512 workgroups (256 clips: every
    launch at one to three row groups; 64 clips and fewer: none); four row groups and the small batches stay on the 128-column
    form or off the f16 kernel altogether; the override 1 never gives the wide form, the override 2 gives it wherever the f16
    kernel runs and supports it."""
    for name, (N, K) in LAYERS.items():
        auto = conv_tile(0, B, rg, N, K)
        want_wide = rg <= 3 and B == 256
        runs_h2 = (N // 128) * B >= 128
        assert auto == (0 if not runs_h2 else 2 if want_wide else 1), (name, B, rg)
        assert conv_tile(1, B, rg, N, K) == (1 if runs_h2 else 0)
        assert conv_tile(2, B, rg, N, K) == (0 if not runs_h2 else 2 if rg <= 3 else 1)


@pytest.mark.parametrize("width", [NARROW, WIDE])
def test_slab_groups(width):
    """Every group size divides the tile count and the group's packed weights fit the budget (a single tile always does:
    256 columns x 1024 x 4 bytes = 1 MiB)."""
    for name, (N, K) in LAYERS.items():
        tiles_n = N // width
        sg = slab_group(tiles_n, width, K)
        assert 1 <= sg <= tiles_n and tiles_n % sg == 0, (name, width, sg)
        assert sg * width * K * WEIGHT_BYTES <= L2_BUDGET, (name, width, sg)
    # the groups of the two 1024 x 1024 launches: 6 of 8 narrow slabs fit -> groups of 4; 3 of 4 wide slabs fit -> groups of 2
    assert slab_group(8, NARROW, 1024) == 4 and slab_group(4, WIDE, 1024) == 2
    assert slab_group(4, WIDE, 512) == 4 and slab_group(2, WIDE, 1024) == 2 and slab_group(2, WIDE, 128) == 2


def test_every_clip_and_tile_is_walked_once():
    """The XCD walk of conv_block_uniform restated: block id -> (clip, tile) is a bijection for both widths."""
    for width in (NARROW, WIDE):
        for B in (8, 16, 64, 256):
            for name, (N, K) in LAYERS.items():
                tiles_n = N // width
                ntiles = tiles_n * B
                seen = set()
                for bid in range(ntiles):
                    if ntiles % 8 == 0:
                        x, j, R = bid & 7, bid >> 3, ntiles >> 3
                        nclip = R // tiles_n
                        if nclip * tiles_n == R and nclip > 0:
                            sg = slab_group(tiles_n, width, K)
                            grp, r = divmod(j, nclip * sg)
                            clip, slab = x * nclip + r // sg, grp * sg + r % sg
                        else:
                            clip, slab = divmod(x * R + j, tiles_n)
                    else:
                        clip, slab = divmod(bid, tiles_n)
                    assert 0 <= clip < B and 0 <= slab < tiles_n
                    seen.add((clip, slab))
                assert len(seen) == ntiles, (width, B, name)
