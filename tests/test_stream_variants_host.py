"""Which analysis and synthesis run lengths the batches of tests/test_gpu_stream_variants.py select (no device): the rule of
analysis_run_for (csrc/batch_layout.hpp) restated, uniform step included, and held against the C rule itself through
tests/host_sim/batch_layout_check.cpp; the batches that select the analysis runs 5, 6, 8, 10 and 11; and the record that every
batch of the tests that ran the wide-band, L1 and unfused streaming kernels before that module selects 4 and 4 (DESIGN.md
section 26)."""
import importlib

import pytest

from test_batch_layout_host import batch_layout_check, case_line, cases
from test_loop_run_rule_host import BATCHES, HEAD, KHOP, expected_synth_run

STREAM_WAVES = 4          # runs of one clip per workgroup of the streaming kernels (kStreamWaves)


def expected_analysis_run(lengths):
    """Frames per analysis run: the longest R in 12 .. 4 that still gives 4096 runs over the batch, else 4; for a batch whose
    clips all have the same frame count then the nearest R' in R .. max(4, R - 3) whose run count per clip is a multiple of the
    waves of a workgroup, if there is one."""
    T = [1 + n // KHOP for n in lengths]
    R = 4
    for cand in range(12, 3, -1):
        if sum((t + cand - 1) // cand for t in T) >= 4096:
            R = cand
            break
    if all(t == T[0] for t in T):
        for cand in range(R, max(4, R - 3) - 1, -1):
            if ((T[0] + cand - 1) // cand) % STREAM_WAVES == 0:
                return cand
    return R


# name: (lengths, analysis run, synthesis run).  A<k>: the head clips and 2045 fillers of k hop blocks (k + 1 frames: one run
# of k + 1 .. 12 frames, two of k), which only move the rule; U11: uniform, 126 frames, 12 through the 4096-run rule and 11
# through the multiple-of-four-waves step
NEW_BATCHES = {
    "A5": (HEAD + [1280] * 2045, 5, 6), "A6": (HEAD + [1536] * 2045, 6, 4), "A8": (HEAD + [2048] * 2045, 8, 6),
    "A10": (HEAD + [2560] * 2045, 10, 8), "A11": (HEAD + [2816] * 2045, 11, 8), "U11": ([32000] * 400, 11, 12),
}
OLD_ANALYSIS = {"R12": 12, "R8": 9, "R6": 7, "U12": 12}
# every batch of the device module: name -> (lengths, analysis run, synthesis run)
ALL_BATCHES = dict(NEW_BATCHES, **{name: (lengths, OLD_ANALYSIS[name], run) for name, (lengths, run) in BATCHES.items()})
ALONE = {"head": (HEAD, 4, 4), "one16000": ([16000], 4, 4), "one32000": ([32000], 4, 4), "three16000": ([16000] * 3, 4, 4)}


def test_the_table():
    assert len(ALL_BATCHES) == 10
    for name, (lengths, an, syn) in {**ALL_BATCHES, **ALONE}.items():
        assert (expected_analysis_run(lengths), expected_synth_run(lengths)) == (an, syn), name
        assert lengths[:5] == HEAD or len(set(lengths)) == 1, name
    for k in range(5, 12):
        assert expected_analysis_run(HEAD + [KHOP * k] * 2045) == k


def test_the_device_batches_select_every_analysis_run():
    runs = {an for _, an, _ in list(ALL_BATCHES.values()) + list(ALONE.values())}
    assert runs == set(range(4, 13))
    assert {syn for _, _, syn in list(ALL_BATCHES.values()) + list(ALONE.values())} == {4, 6, 8, 12}
    # ... and production batches the rule was measured on
    assert expected_analysis_run([48000] * 256) == 12 and expected_analysis_run([48000] * 64) == 4


def test_the_restatements_against_the_c_rule():
    """expected_analysis_run and expected_synth_run against analysis_run_for / synth_run_for on every accepted card case of
    test_batch_layout_host.cases() and on the new batches."""
    todo = {name: lengths for name, (route, lengths, off) in cases().items() if route == "card" and off is None}
    todo.update({name: lengths for name, (lengths, _, _) in {**NEW_BATCHES, **ALONE}.items()})
    got = batch_layout_check()("".join(case_line("card", lengths, None) for lengths in todo.values()))
    assert len(got) == len(todo)
    accepted = 0
    for (name, lengths), g in zip(todo.items(), got):
        assert (g["rc"] == -1) == ("refuse" in name), name
        if g["rc"] != 0:
            continue
        accepted += 1
        assert expected_analysis_run(lengths) == g["an_run"], name
        assert expected_synth_run(lengths) == g["synth_run"], name
    assert accepted >= 20
    by = dict(zip(todo, got))
    for name, (lengths, an, syn) in NEW_BATCHES.items():
        assert (by[name]["an_run"], by[name]["synth_run"]) == (an, syn), name
    # the uniform step is what moves these two: without it the 4096-run rule alone gives 12
    assert by["card_400x32000"]["an_run"] == by["U11"]["an_run"] == 11 and by["U11"]["T"][0] == 126
    assert sum((126 + 11) // 12 for _ in range(400)) >= 4096 and ((126 + 11) // 12) % STREAM_WAVES != 0 and ((126 + 10) // 11) % STREAM_WAVES == 0


def test_the_head_clips_runs():
    """What a run length changes for the compared clips: the analysis runs of each head clip and where its last run ends."""
    T = [1 + n // KHOP for n in HEAD]
    assert T == [73, 63, 32, 94, 3]
    assert [[(t + r - 1) // r for t in T] for r in (5, 11, 12)] == [[15, 13, 7, 19, 1], [7, 6, 3, 9, 1], [7, 6, 3, 8, 1]]
    # the last run of a clip is partly filled at every run length but for 32 frames at run 8 and 63 at runs 7 and 9
    assert [t % r for r in (5, 6, 7, 8, 9, 10, 11, 12) for t in T[:4]].count(0) == 3


# ---- the gap -------------------------------------------------------------------------------------------------------------------
WIDE_BAND = [[16000, 23456, 48000], [48000] * 4, [16000] * 32, [16000, 160000, 48000, 23456, 100001, 64000, 32000, 128000], [16000] * 2,
             [16000, 48000, 23456], [16000] * 4, [16000, 16000, 48000], [16000], [16000] * 6 + [48000, 23456]]     # test_gpu_wide_band.py
SEAM_L1 = [[16000]]                                   # test_gpu_seam.py::test_push_extremes_l1_extension
PAYLOAD_L1 = [[16000] * 32]                           # test_gpu_payload_length.py::test_push_extremes_l1_first_gradient_at_64_bits
DETECTOR_SIZES = [[16000] * 32, [16000] * 256, [16000, 160000, 48000, 23456], [16000], [16000, 24000]]      # test_gpu_detector_sizes.py


def older_lists():
    found = [(f"wide_band {v}", v) for v in WIDE_BAND] + [(f"seam {v}", v) for v in SEAM_L1] + [(f"payload {v}", v) for v in PAYLOAD_L1] + \
            [(f"detector_sizes {v[:4]} ({len(v)})", v) for v in DETECTOR_SIZES]
    for m in ("test_gpu_payload_length", "test_gpu_detector_sizes"):
        found.append((f"{m}.RAGGED", list(importlib.import_module(m).RAGGED)))
    return found


def test_every_batch_of_the_older_variant_tests_selects_4_and_4():
    """The gap this records: the wide-band kernels, the L1 kernels and the unfused narrow pair never left run 4 before
    test_gpu_stream_variants.py."""
    found = older_lists()
    assert len(found) >= 19
    for name, lengths in found:
        assert expected_synth_run(lengths) == 4, name
        assert expected_analysis_run(lengths) == 4, name


@pytest.mark.parametrize("lengths,an", [([48000] * 256, 12), ([48000] * 128, 6), ([16000] * 683, 12), ([1280] * 2048, 5), ([1024] * 2048, 4)])
def test_the_rule_where_it_is_easy_to_read(lengths, an):
    """256 x 3 s: 188 frames, 16 runs of 12 each, 4096 in all, and 16 is a multiple of four; 128 x 3 s: 2048 runs of 12, 4096
    from 6 on (32 per clip); 2048 clips of 6 frames: two runs of 5 each, and no run of 5 .. 4 frames makes that a multiple of
    four, so the uniform step leaves it."""
    assert expected_analysis_run(lengths) == an
