"""CPU test of polar_exact (aware_amd/csrc/polar.hpp, no GPU): the magnitude and unit phasor the analysis stores for the
original audio, through tests/host_sim/polar_check.cpp, which models the hardware square root and reciprocal as flushing
subnormal operands and results and sweeps the components over exponents -149 .. +60 against hypot and atan2 in double."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "host_sim", "polar_check.cpp")
    exe = str(tmp_path_factory.mktemp("polar") / "polar_check")
    # no contraction: the plain form and polar_exact must round the sum of squares alike, as the check compares their bits
    subprocess.run(["c++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, src], check=True)
    tok = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    out = dict(zip(tok[0::2], map(float, tok[1::2])))
    print(out)
    return out


def test_no_bin_is_lost(report):
    """Every non-zero bin of the sweep gets a magnitude above zero; the plain form on the same model loses every bin whose
    sum of squares is subnormal (so the model does show the fault this helper is there for); (0, 0) and (-0, 0) give 0."""
    assert report["n"] > 400000
    assert report["lost"] == 0
    assert report["plain_lost"] > 0.25 * report["n"]
    assert report["zero_mag"] == 1


def test_magnitude_and_phasor_against_double(report):
    assert report["mag_ulp"] <= 2.0
    assert report["norm"] < 1e-6
    assert report["phase"] < 1e-6


def test_bits_of_the_plain_form_from_2_pow_minus_100_on(report):
    assert report["compared"] > 0.25 * report["n"]
    assert report["differs"] == 0
