"""Which synthesis run length a batch selects (no device): the rule of aware_batch_create (synth_run_for and
run_cuts_short_segments, csrc/batch_layout.hpp) restated, the batches of tests/test_gpu_loop_run_lengths.py that select 12, 8
and 6, and the record that every batch of the other loop-chain device tests selects 4.
tests/test_batch_layout_host.py holds the restatement against the C rule itself."""
import importlib

import pytest

KHOP = 256
HEAD = [18432, 16000, 8000, 24000, 513]
# name: (lengths, the run aware_batch_create picks); the fillers behind the head clips only move the rule
BATCHES = {"R12": (HEAD + [3328] * 2041, 12), "R8": (HEAD + [2304] * 2045, 8), "R6": (HEAD + [1792] * 2046, 6), "U12": ([16000] * 683, 12)}
LOOP_MODULES = ["attacks", "reverb", "speed", "stretch", "pitch", "pv", "delete", "mixture", "gain", "filter"]
CONSTANTS = ["SHORT", "LONG", "RAGGED", "TINY", "UNIFORM"]
# the lengths lists those modules spell out inside their tests
LITERALS = [[16000] * 8, [16000, 40000, 64000], [16000, 16000 + 256 * 9], [16000, 20000], [16000, 40000, 64000, 8000], [16000, 24000],
            [16000] * 4, [16000, 40000], [8000, 16000, 24000], [16000, 8000, 24000], [8000, 16000], [16000, 8000, 16000, 8000],
            [16000, 8000], [16000, 8000, 513], [16000] * 2, [8000] * 2]


def expected_synth_run(lengths):
    """Hop blocks per synthesis run: the longest of 12 / 8 / 6 / 4 that still gives 4096 runs over the batch, else the shortest
    one allowed; a length is not allowed if it would cut some clip into several segments of fewer than 3 blocks (the staged
    adjoint folds the reflect pads inside the first and last segment); 16 if none is allowed."""
    run = 16
    for rb in (12, 8, 6, 4):
        runs = sum((n // KHOP + rb - 1) // rb for n in lengths)
        ok = True
        for n in lengths:
            nb = n // KHOP
            ns = (nb + rb - 1) // rb
            if ns > 1 and nb // ns < 3:
                ok = False
        if not ok:
            continue
        run = rb
        if runs >= 4096:
            break
    return run


def segments(n, run):
    """Hop blocks of each workgroup segment of a clip (synth_segment in csrc: nb blocks split as evenly as possible)."""
    nb = n // KHOP
    ns = max(1, (nb + run - 1) // run)
    return [nb // ns + (1 if s < nb % ns else 0) for s in range(ns)]


@pytest.mark.parametrize("lengths,run", [([48000] * 256, 12), ([48000] * 128, 6), ([48000] * 64, 4)] + list(BATCHES.values()),
                         ids=["bench256", "bench128", "bench64"] + list(BATCHES))
def test_the_rule_on_production_and_test_batches(lengths, run):
    assert expected_synth_run(lengths) == run


def test_the_exclusion():
    """A 5-block clip cannot be cut into runs of 4 (segments of 3 and 2 blocks): such a batch stays at 6."""
    assert expected_synth_run([1300]) == 6 and expected_synth_run([1300, 16000]) == 6
    assert expected_synth_run([1024]) == 4 and expected_synth_run([1536]) == 4


def test_the_head_clips_segments_at_run_12():
    assert [segments(n, 12) for n in HEAD] == [[12] * 6, [11, 11, 10, 10, 10, 10], [11, 10, 10], [12] * 5 + [11] * 3, [2]]
    assert segments(16000, 4) == [4] * 14 + [3] * 2          # at run 4 no segment exceeds 1024 samples


def existing_lists():
    found = []
    for m in LOOP_MODULES:
        mod = importlib.import_module(f"test_gpu_loop_{m}")
        for c in CONSTANTS:
            if hasattr(mod, c):
                found.append((f"{m}.{c}", list(getattr(mod, c))))
    return found


def test_every_batch_of_the_older_loop_tests_selects_run_4():
    """The gap this records: the loop-chain device tests before test_gpu_loop_run_lengths.py never left run 4."""
    found = existing_lists()
    assert len(found) >= 20
    for name, lengths in found + [(str(v), v) for v in LITERALS]:
        assert expected_synth_run(lengths) == 4, name
