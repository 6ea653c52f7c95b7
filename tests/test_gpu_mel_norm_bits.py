"""The bits of the detector's mel stage (InstanceNorm1d over time, GlobalStandardize per clip, AvgPool1d(2, 2) and their
backward): csrc/mel_norm.hpp and the kernels that call it -- the chunked family and the clip kernels of
csrc/detector_kernels.hip, mel_front_x3_kernel and mel_back_x3_kernel of csrc/gemm_x3.hip.  The other suites compare these to
float64 within a tolerance only.

tests/golden/mel_norm_sha256.json was recorded with tools/detector_sizes_bench.py (dump_bits) on the device with aware_amd/csrc/
as it was before the stage's maths moved into csrc/mel_norm.hpp and the any-bank twins of the chunked kernels became
instantiations of one family (the tree of the commit "Loop stage kernels: one prologue, one resampler entry, one OLA, one
draw").  The record can be checked: put that commit's aware_amd/csrc/ under this test, the tool and the fixture, build, and run
the test; it passes there as it does here.  A reordered sum or a changed contraction into FMAs changes a hash.  The fixture also
holds the sha256 of every case's inputs, so a changed input (another numpy stream, other weights) is told apart from a changed
kernel.

Detectors: the card's (128 bands) and mel banks of 13, 200, 300 and 512 bands (one partial group of 128 channels, two, three,
four full ones), the latter with one 64-channel block and 8 bits.  Ragged batches with T = 3, 63, 64, 192 frames (clip form up
to its limit) and T = 3, 63, 193, 225, 224 (chunked form: clips that leave most chunks at once, last chunks of one frame and of
32, unpaired last frames); the shortest clip, 600 samples, is accepted as it stands.  Uniform batches of 192 clips of T = 63
and 161 for the card's detector (the one-launch front and back kernels).  The embed loop's first gradient on
[16000, 12000, 9000].

Run on the MI355X box:  python -m pytest tests/test_gpu_mel_norm_bits.py -m gpu -q -s"""
import importlib.util
import json
import os
import re

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tool():
    from aware_amd._lib import require_gpu
    require_gpu()
    spec = importlib.util.spec_from_file_location("detector_sizes_bench", os.path.join(ROOT, "tools", "detector_sizes_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "mel_norm_sha256.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got(tool):
    return tool.dump_bits()


def constant(source, name):
    with open(os.path.join(ROOT, "aware_amd", "csrc", source)) as f:
        return int(re.search(rf"constexpr int {name} = (\d+);", f.read()).group(1))


def entry_plan_args(entry):
    """(pipe, readout, training) that the C entry point `entry` hands to det_plan (capi.hip)."""
    with open(os.path.join(ROOT, "aware_amd", "csrc", "capi.hip")) as f:
        body = f.read().split(f'extern "C" int {entry}(')[1].split('extern "C"')[0]
    pipe, readout, training = re.search(r"det_plan\(d, b, (\d), (\d), (true|false),", body).groups()
    return int(pipe), int(readout), training == "true"


def mel_kinds(ch, stride, card_arch, T, pipe, training, min_clips):
    """det_plan's rules for the mel stage (capi.hip), every condition restated in what Python sees: (MelFwd::Front,
    Conv::MelBack) for a detector of stored channels `ch` on rows of `stride` floats and a batch of frame counts `T`.
    Sufficient conditions: the block above block 0 is only looked at where it certainly runs a fused kind."""
    melTpk = ch[0] % 128 == 0                                   # detector_upload packs the mel operand for the x3 kernels
    wTpk0 = ch[0] % 128 == 0 and ch[1] % 64 == 0                # ... and block 0's transposed weights
    supported = 2 <= T[0] <= 192 and stride % 64 == 0 and stride % 4 == 0       # mel_front_x3_supported(T, K, lda)
    front = pipe != 1 and ch[0] == 128 and melTpk and len(set(T)) == 1 and len(T) >= min_clips and supported
    tp = T[0] // 2 if len({t // 2 for t in T}) == 1 else 0      # aware_batch::uniform_tp, clip_tile_groups
    nwm = (tp + 31) // 32 if tp and (tp + 31) // 32 <= 4 else 0
    # dz[0]: block 1's data gradient is a clip-aligned kind (card blocks, uniform batch, 128 channels or more) and block 0 is
    # not the top of the backward loop, with or without the fused read-out (three blocks or more)
    dz0 = card_arch and nwm > 0 and len(ch) - 1 >= 3 and ch[1] >= 128
    back = front and dz0 and not training and wTpk0 and ch[1] % 64 == 0 and ch[0] == 128
    return front, back


def test_the_batches_take_the_kernels_they_are_meant_for(tool):
    """det_plan's conditions (capi.hip), restated: the ragged batches stay below / go above kMelClipFrames with the frame
    counts the docstring lists; the uniform batches satisfy every condition of MelFwd::Front in aware_detector_forward and
    aware_detector_backward and of Conv::MelBack in the latter (mel_kinds, with the arguments the entry points hand to
    det_plan), at two instantiations each of mel_front_x3_kernel<(T + 31) / 32> and mel_back_x3_kernel<((T + 1) / 2 + 31) / 32>;
    a ragged batch of the same detector satisfies neither."""
    from aware_amd import runtime as rt
    from aware_amd.detection import AWAREDetectorNet
    from aware_amd.utils.audio import default_plan
    clip_frames = constant("kernels.h", "kMelClipFrames")
    frames = lambda lengths: [1 + n // 256 for n in lengths]
    assert frames(tool.BITS_RAGGED["clip"]) == [3, 63, 64, 192] and max(frames(tool.BITS_RAGGED["clip"])) == clip_frames
    assert frames(tool.BITS_RAGGED["chunked"]) == [3, 63, 193, 225, 224] and min(frames(tool.BITS_RAGGED["chunked"])[2:]) > clip_frames
    assert tool.BITS_DETECTORS["card"] == {}
    assert [kw["n_mels"] for k, kw in tool.BITS_DETECTORS.items() if k != "card"] == [13, 200, 300, 512]
    min_clips = constant("capi.hip", "kMelFrontMinClips")
    plan, net = default_plan(), AWAREDetectorNet()
    det = net.device_weights(plan)
    ch = rt.stored_channels(net.channels)
    assert ch == list(det.channels) and det.is_card
    fwd_pipe, _, fwd_training = entry_plan_args("aware_detector_forward")
    bwd_pipe, _, bwd_training = entry_plan_args("aware_detector_backward")
    front, back = set(), set()
    for lengths in tool.BITS_UNIFORM.values():
        T = frames(lengths)
        assert mel_kinds(ch, plan.band_stride, det.is_card, T, fwd_pipe, fwd_training, min_clips)[0]
        assert mel_kinds(ch, plan.band_stride, det.is_card, T, bwd_pipe, bwd_training, min_clips) == (True, True)
        front.add((T[0] + 31) // 32)
        back.add(((T[0] + 1) // 2 + 31) // 32)
    assert len(front) == 2 and len(back) == 2
    for lengths in tool.BITS_RAGGED.values():
        assert mel_kinds(ch, plan.band_stride, det.is_card, frames(lengths), bwd_pipe, bwd_training, min_clips) == (False, False)


def test_inputs_are_the_recorded_ones(got, want):
    assert got["inputs"] == want["inputs"]


def test_mel_stage_keeps_its_bits(got, want):
    """Every detector on both ragged batches, the card's on both uniform batches, and the loop's first gradient."""
    cases = [f"{d}/{b}" for d in ("card", "m13", "m200", "m300", "m512") for b in ("clip", "chunked")]
    cases += ["card/u63", "card/u161", "embed"]
    assert sorted(got["sha256"]) == sorted(want["sha256"]) == sorted(cases)
    for case in cases:
        assert got["inputs"][case] == want["inputs"][case], f"{case}: the inputs differ, not the kernels"
        assert got["sha256"][case] == want["sha256"][case], case
