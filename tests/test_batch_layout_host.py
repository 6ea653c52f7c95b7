"""The layout of a batch (no device): csrc/batch_layout.hpp -- the per-clip tables of aware_batch_create and
aware_batch_create_for_plan, the card route's run lengths and workgroup tables -- through tests/host_sim/batch_layout_check.cpp
against what the two constructors computed before that arithmetic moved into the header (tests/golden/batch_layout.json), and
the Python restatement of the synthesis run rule (test_loop_run_rule_host.expected_synth_run) against the C rule itself."""
import json
import os
import shutil
import struct
import subprocess
import zlib

from test_loop_run_rule_host import BATCHES, HEAD, expected_synth_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = ["NF", "NP", "NS", "max_frames", "max_len", "pstride", "uniform_tp", "synth_run", "an_run", "n_an_wg", "n_syn_wg"]


def _at_4096(lengths):
    """Each clip at the next multiple of 4096 behind the clip before it."""
    offs, at = [], 0
    for n in lengths:
        offs.append(at)
        at = (at + n + 4095) // 4096 * 4096
    return offs


def cases():
    """name -> (route arguments, lengths, in_offsets or None): the smallest batches at which each branch can go wrong."""
    card = {
        "513": [513], "1024": [1024], "1300": [1300], "1536": [1536], "1300_16000": [1300, 16000], "16000_8000_513": [16000, 8000, 513],
        "head": HEAD, "4x16000": [16000] * 4, "64x48000": [48000] * 64, "128x48000": [48000] * 128, "256x48000": [48000] * 256,
        "400x32000": [32000] * 400,          # uniform: the multiple-of-kStreamWaves step moves the analysis run from 12 to 11
        "long": [16777216],                  # the guard skips the workgroup tables
        "refuse_512": [512], "refuse_16000_512": [16000, 512],
    }
    card.update({name: lengths for name, (lengths, _) in BATCHES.items()})
    out = {f"card_{k}": ("card", v, None) for k, v in card.items()}
    out["card_head_offsets"] = ("card", HEAD, _at_4096(HEAD))
    for n_fft, hop in ((256, 64), (512, 128), (1024, 256), (2048, 512), (4096, 1024)):
        g = f"gen {n_fft} {hop}"
        out[f"gen{n_fft}_shortest"] = (g, [n_fft // 2 + 1], None)
        out[f"gen{n_fft}_ragged"] = (g, [4 * n_fft + 37, n_fft // 2 + 1, 16000, 9 * hop], None)
        out[f"gen{n_fft}_uniform"] = (g, [16000] * 8, None)
        out[f"gen{n_fft}_refuse"] = (g, [n_fft // 2], None)
    return out


def case_line(route, lengths, offsets):
    nums = list(lengths) + list(offsets or [])
    return f"{route} {len(lengths)} {1 if offsets else 0} " + " ".join(map(str, nums)) + "\n"


def condense(got, B):
    """What the golden file keeps of one result: everything for at most 8 clips, else the scalars and a CRC32 of each table
    (its values as little-endian int32)."""
    if got["rc"] != 0 or B <= 8:
        return got
    out = {k: v for k, v in got.items() if not isinstance(v, list)}
    out["crc32"] = {k: zlib.crc32(struct.pack(f"<{len(v)}i", *v)) for k, v in got.items() if isinstance(v, list)}
    return out


def batch_layout_check():
    """tests/host_sim/batch_layout_check.cpp, built without HIP where it is missing or older than its sources.  Returns
    run(text) -> one dict per line of `text`."""
    exe = os.path.join(ROOT, "tests", "host_sim", "batch_layout_check")
    src = os.path.join(ROOT, "tests", "host_sim", "batch_layout_check.cpp")
    hdr = os.path.join(ROOT, "aware_amd", "csrc", "batch_layout.hpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        cxx = ["g++", "-O2", "-std=c++17"] if shutil.which("g++") else ["hipcc", "-O2", "-std=c++17", "-x", "hip", "--offload-host-only"]
        subprocess.run(cxx + ["-o", exe, src], check=True)

    def run(text):
        out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout
        return [json.loads(line) for line in out.splitlines()]

    return run


def test_layout_matches_the_constructors_it_came_from():
    with open(os.path.join(ROOT, "tests", "golden", "batch_layout.json")) as f:
        golden = json.load(f)
    cs = cases()
    assert sorted(golden) == sorted(cs)
    got = batch_layout_check()("".join(case_line(*c) for c in cs.values()))
    assert len(got) == len(cs)
    for (name, (route, lengths, _)), g in zip(cs.items(), got):
        assert condense(g, len(lengths)) == golden[name], name
        assert (g["rc"] == -1) == ("refuse" in name), name
        if g["rc"] == 0:
            assert set(SCALARS[:7]) <= set(g) and (route != "card" or set(SCALARS) <= set(g)), name
        # the restatement in Python against the C rule it restates
        if route == "card" and g["rc"] == 0:
            assert expected_synth_run(lengths) == g["synth_run"], name
    # what the cases are there for
    by = dict(zip(cs, got))
    assert by["card_1300"]["synth_run"] == 6 and by["card_1300_16000"]["synth_run"] == 6          # the exclusion
    assert by["card_400x32000"]["T"][0] == 126 and by["card_400x32000"]["an_run"] == 11
    assert by["card_long"]["n_an_wg"] == 0 and by["card_long"]["n_syn_wg"] == 0
    assert by["card_head_offsets"]["in_off"] == [0, 20480, 36864, 45056, 69632]
