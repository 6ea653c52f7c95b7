"""CPU test of where the wave-level FFT (aware_amd/csrc/fft512.hpp) keeps its values in LDS (no GPU): tests/host_sim/
lds_bank_sim.cpp evaluates the index functions of both exchanges and of the twiddle / window / merge tables for lanes 0..63
under the banking rule of the instruction that moves each (MI355X: ds_read_b64 in 32-lane halves on 64 banks, ds_write_b64
in 16-lane groups on 32 banks) and counts the extra cycles of every bank conflict; it also checks, on the same functions,
that each exchange is the transpose tests/host_sim/fft_sim.cpp verifies numerically.  The rows marked "(former layout)"
restate what the layouts and the paired loads before cost, for the record; they are printed, not asserted."""
import os
import subprocess

from conftest import ROOT

EXCHANGES = ["xch1_store", "xch1_load", "xch2_store", "xch2_load"]
TABLES = ["tw1s", "tw2s", "wins / mcs"]


def test_exchanges_and_tables_are_conflict_free(tmp_path):
    src = os.path.join(ROOT, "tests", "host_sim", "lds_bank_sim.cpp")
    exe = str(tmp_path / "lds_bank_sim")
    subprocess.run(["hipcc", "-O2", "-x", "hip", "--offload-host-only", "-o", exe, src], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    print(res.stdout)
    rows, tail = {}, {}
    for line in res.stdout.strip().splitlines():
        if " accesses " in line:
            name = line[:28].strip()
            tok = line[28:].split()
            rows[name] = dict(instr=tok[0], cycles=int(tok[tok.index("cycles") + 1]), conflict=int(tok[tok.index("conflict_cycles") + 1]),
                              former="(former" in line)
        else:
            k, v = line.split()
            tail[k] = int(v)
    for name in EXCHANGES + TABLES:
        assert not rows[name]["former"]
        assert rows[name]["conflict"] == 0, (name, rows[name])
        assert rows[name]["instr"] == ("ds_write_b64" if name.endswith("_store") else "ds_read_b64")
    assert tail == {"permutation_errors": 0, "asserted_conflict_cycles": 0}
    assert res.returncode == 0
    # the model tells a conflicting layout from a clean one: the former exchange-2 store met 2-way once per 16-lane group,
    # the former [n0][q0] twiddle table 4-way under the paired load's rule and 2-way under ds_read_b64's
    assert rows["old xch2_store"]["conflict"] == 8 * 4
    assert rows["old tw2s"]["conflict"] == 7 * 4 * 3 and rows["old tw2s as ds_read_b64"]["conflict"] == 7 * 2
    # LDS cycles of the loads of one frame's transform: 38 single loads against the same values in pairs
    new = sum(rows[n]["cycles"] for n in ["xch1_load", "xch2_load", "tw1s", "tw2s", "wins / mcs"])
    old = sum(rows[n]["cycles"] for n in ["old xch1_load", "old xch2_load", "old tw1s", "old tw2s", "old wins / mcs"])
    assert new == 38 * 2 and old >= 2 * new
