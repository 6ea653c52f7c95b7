"""The bits of the embed loop's stage kernels (csrc/loop_speed_kernels.hip, loop_stretch_kernels.hip, loop_pitch_kernels.hip,
loop_delete_kernels.hip, loop_filter_kernels.hip) that no other record holds: the stand-alone entries, which the other suites
compare to the float64 restatement within a tolerance only, and the band-filter chains inside the loop.

tests/golden/loop_stage_sha256.json was recorded with tools/loop_attack_bench.py (dump_alone and dump) on the device with
aware_amd/csrc/ and aware_amd/runtime.py as they were before the stage kernels' shared code moved into csrc/loop_stage.hpp
and csrc/ola.hpp (the tree of the commit "Scan long recordings: find watermarked spans and read their payloads").  The record
can be checked: put that commit's aware_amd/csrc/ and aware_amd/runtime.py under this test, the tool and the fixture, build,
and run the test; it passes there as it does here.  A reordered sum, another rounding or a moved clamp changes a hash.

Shapes: stand-alone clips of 4099 and 7937 samples packed back to back (an odd second offset, several workgroups per clip); in
the loop the ragged batch [16000, 12000, 9000] of tests/golden/loop_chains_sha256.json, 8 iterations.

Run on the MI355X box:  python -m pytest tests/test_gpu_loop_stage_bits.py -m gpu -q -s"""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tool():
    from aware_amd._lib import require_gpu
    require_gpu()
    spec = importlib.util.spec_from_file_location("loop_attack_bench", os.path.join(ROOT, "tools", "loop_attack_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "loop_stage_sha256.json")) as f:
        return json.load(f)


def test_stand_alone_entries_keep_their_bits(tool, want):
    """Forward and adjoint of aware_speed_change, aware_pitch_shift_ola and aware_stretch_ola at the ends of their ranges, at
    -1, 0, 1 and 3000, with outputs of the clip's own and of the true length (so the adjoint's two sides differ in length);
    aware_delete_samples at four cuts in both directions; aware_band_filter's four responses and their taps."""
    got = tool.dump_alone()
    assert sorted(got) == sorted(want["alone"]) and len(got) == 3 * 6 * 2 * 2 + 4 * 2 + 4 * 2
    for name in sorted(got):
        assert got[name] == want["alone"][name], name


def test_filter_chains_keep_their_bits(tool, want):
    """Every chain of FILTER_VARIANTS: coefficients, best coefficients, losses and the finished waveform after 8 iterations."""
    from aware_amd.utils.models import load
    chains = want["chains"]
    assert chains["names"] == list(tool.FILTER_VARIANTS) and chains["lengths"] == [16000, 12000, 9000] and chains["iters"] == 8
    emb, _ = load()
    emb.verbose = False
    got = tool.dump(emb, None, names=chains["names"], lengths=chains["lengths"], iters=chains["iters"])
    for name in chains["names"]:
        assert got[name] == chains["sha256"][name], name
