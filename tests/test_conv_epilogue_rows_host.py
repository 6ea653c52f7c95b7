"""CPU test of the layout algebra behind the wide conv form's row-major epilogue (aware_amd/csrc/conv_epilogue_rows.hpp, no
GPU): the four lane -> LDS maps walked by tests/host_sim/conv_epilogue_rows_check.cpp for RG = 1, 2, 3, and the launcher's
choice of form for aligned and unaligned buffers."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

MAPS = ("c_write", "c_read", "act_write", "act_read")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "host_sim", "conv_epilogue_rows_check.cpp")
    exe = str(tmp_path_factory.mktemp("rows") / "conv_epilogue_rows_check")
    subprocess.run(["c++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                   check=True)
    out = {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines():
        tok = line.split()
        vals = dict(zip(tok[0::2], tok[1::2]))
        out[(int(vals["RG"]), vals["map"])] = {k: float(vals[k]) for k in ("bijection", "owner", "ways64", "wayshw")}
    return out


def test_every_map_reported(report):
    assert set(report) == {(rg, m) for rg in (1, 2, 3) for m in MAPS}


@pytest.mark.parametrize("RG", [1, 2, 3])
@pytest.mark.parametrize("name", MAPS)
def test_map_is_a_bijection_onto_the_region(report, RG, name):
    assert report[(RG, name)]["bijection"] == 1


@pytest.mark.parametrize("RG", [1, 2, 3])
@pytest.mark.parametrize("name", MAPS)
def test_turn_returns_each_element_to_its_owner(report, RG, name):
    """The slot a map uses for element (row, col) is the slot from which the other layout's map takes that (row, col)."""
    assert report[(RG, name)]["owner"] == 1


@pytest.mark.parametrize("RG", [1, 2, 3])
@pytest.mark.parametrize("name", MAPS)
def test_at_most_two_way_bank_conflicts(report, RG, name):
    """No wave instruction worse than 2-way: counted over all 64 lanes on 64 banks of 4 bytes, and per lane group as the
    hardware serves the instruction (where the maps are free of conflicts)."""
    print(RG, name, report[(RG, name)])
    assert report[(RG, name)]["ways64"] <= 2
    assert report[(RG, name)]["wayshw"] <= 2


def test_launcher_reports_the_form():
    """aware_gemm_clip_h2_form: 1 for the 128-column form, 3 (row-major epilogue) for the wide form on 16-byte aligned buffers
    with ldc % 4 == 0, 2 (accumulator-layout epilogue) when ldc, C or -- data gradient only -- act are not."""
    from aware_amd._lib import load_library
    lib = load_library()
    form = lib.aware_gemm_clip_h2_form
    C, act = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)
    N, K, Tp = 512, 128, 94
    for epi, last in ((0, 0), (1, 0), (2, 0), (1, 1)):
        assert form(C, N, act, Tp, N, K, K, epi, last, 1) == 1
        assert form(C, N, act, Tp, N, K, K, epi, last, 0) == 1
        assert form(C, N, act, Tp, N, K, K, epi, last, 2) == 3
        assert form(C, N + 4, act, Tp, N, K, K, epi, last, 2) == 3
        for ldc in (N + 1, N + 2, N + 3):
            assert form(C, ldc, act, Tp, N, K, K, epi, last, 2) == 2
        assert form(ctypes.c_void_p(0x10004), N, act, Tp, N, K, K, epi, last, 2) == 2
        assert form(C, N, ctypes.c_void_p(0x20008), Tp, N, K, K, epi, last, 2) == (2 if epi == 2 else 3)
    assert form(C, N, act, 100, N, K, K, 1, 0, 2) == -2          # four row groups: no wide form
    assert form(C, 128, act, Tp, 128, K, K, 1, 0, 2) == -2       # N no multiple of 256
    assert form(None, N, act, Tp, N, K, K, 1, 0, 2) == -1
