"""The twelve loop attack kinds against tests/golden/loop_kinds_table.json, recorded from parse_chain, device_entries_ex,
check_lengths and tests/host_sim/loop_chain_check before the kinds were stated in one table per language
(embedding/loop_attacks.py::TABLE, csrc/loop_limits.hpp::kLoopKindTable): every message, parsed dict, device tuple, return code
and byte count is the recorded one, exactly.  Then the table's own invariants.  No GPU."""
import json
import os
import re

import pytest

import test_loop_attacks_host as H
from conftest import ROOT
from aware_amd.embedding import loop_attacks as LA

with open(os.path.join(ROOT, "tests", "golden", "loop_kinds_table.json")) as _f:
    TABLE = json.load(_f)
NAMES = list(TABLE["entries"])


def _floats(x):
    """The fixture's "nan", "inf" and "-inf" as floats, which JSON cannot hold."""
    if isinstance(x, str) and x in ("nan", "inf", "-inf"):
        return float(x)
    if isinstance(x, list):
        return [_floats(v) for v in x]
    if isinstance(x, dict):
        return {k: _floats(v) for k, v in x.items()}
    return x


def _same(a, b):
    """Equal values of equal types all the way down: a scalar that stayed a scalar, a float that is no int; tuples as lists."""
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    return type(a) is type(b) and a == b


def _result(fn, *args):
    try:
        fn(*args)
        return "ok"
    except ValueError as err:
        return str(err)


def test_the_fixture_is_what_the_issue_asked_for():
    assert len(NAMES) == 12 and len(TABLE["pairs"]) == 144 + 36 + 1
    assert {tuple(c["chain"]) for c in TABLE["pairs"]} >= {(a, b) for a in NAMES for b in NAMES}
    with open(os.path.join(ROOT, "tests", "golden", "loop_chain_messages.json")) as f:
        assert list(TABLE["entries"].items())[:8] == list(json.load(f)["entries"].items())
    assert {f["entry"]["kind"] for f in TABLE["forms"]} == set(NAMES)
    assert {c["chain"][0]["kind"] for c in TABLE["refusals"] if isinstance(c["chain"], list) and c["chain"] and
            isinstance(c["chain"][0], dict) and c["chain"][0].get("kind") in NAMES} == set(NAMES)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "loop_kinds_table.json")) < 256 * 1024


# ---- 1. every case against parse_chain, device_entries_ex and check_lengths --------------------------------------------------
def test_pairs_parse_as_recorded():
    for case in TABLE["pairs"]:
        assert _result(LA.parse_chain, [TABLE["entries"][k] for k in case["chain"]]) == case["result"], case["chain"]


@pytest.mark.parametrize("kind", NAMES)
def test_forms_parse_and_convert_as_recorded(kind):
    forms = [f for f in TABLE["forms"] if f["entry"]["kind"] == kind]
    assert forms
    for form in forms:
        for rate, want in form["rates"].items():
            parsed = LA.parse_chain([form["entry"]], int(rate))
            assert len(parsed) == 1 and _same(parsed[0], want["parsed"]), (form["entry"], rate, parsed)
            k, prob, param = LA.device_entries_ex(parsed, int(rate))[0]
            assert _same([k, prob, list(param)], want["device"]), (form["entry"], rate, k, prob, param)
            assert k == LA.kind_id(kind) == LA.KINDS[kind]


def test_refusals_are_the_recorded_messages():
    for case in TABLE["refusals"]:
        assert _result(LA.parse_chain, _floats(case["chain"]), case["sample_rate"]) == case["result"], case["chain"]
    assert sum(c["result"] != "ok" for c in TABLE["refusals"]) >= 280


def test_check_lengths_messages_are_the_recorded_ones():
    for case in TABLE["check_lengths"]:
        chain = LA.parse_chain(case["chain"], case["sample_rate"])
        assert _result(LA.check_lengths, chain, case["sample_rate"], case["lengths"]) == case["result"], case["chain"]
    assert sum(c["result"] != "ok" for c in TABLE["check_lengths"]) >= 9


# ---- 2. the C parser and carver ----------------------------------------------------------------------------------------------
def test_c_parser_and_carver_answer_as_recorded():
    """Every chain of `pairs`, its entries one by one through device_entries_ex so that a chain parse_chain refuses reaches the
    C parser too (and size_refused_chain its byte count), at the recorded dimensions, ex = 1.  Then the older entry points
    (ex = 0) on every accepted spelling of every kind: they take kinds 0 and 1 and refuse kinds 2 to 11."""
    run = H.loop_chain_check()
    one = {k: LA.device_entries_ex(LA.parse_chain([a]), 16000)[0] for k, a in TABLE["entries"].items()}
    got = run(H._dims_case(TABLE["dims"]) + "".join(H._chain_case([one[k] for k in case["chain"]]) for case in TABLE["pairs"]))
    assert len(got) == len(TABLE["pairs"])
    for case, (rc, nbytes) in zip(TABLE["pairs"], got):
        assert (rc, nbytes) == (case["rc"], case["bytes"]), (case["chain"], rc, nbytes)
        assert (rc == 0) == (case["result"] == "ok")
    forms = [(f["entry"]["kind"], tuple(f["rates"]["16000"]["device"])) for f in TABLE["forms"]]
    long_clip = {"B": 1, "NS": 48128, "NF": 189, "pstride": 16, "out_len": [48000]}      # a second of samples may go
    got = run(H._dims_case(long_clip) + "".join(H._chain_case([e], ex=0) + H._chain_case([e], ex=1) for _, e in forms))
    for (kind, e), (rc0, _), (rc1, _) in zip(forms, got[0::2], got[1::2]):
        assert rc1 == 0 and rc0 == (0 if LA.KINDS[kind] < 2 else -1), (kind, e, rc0, rc1)
    assert sorted({LA.KINDS[kind] for kind, _ in forms}) == list(range(12))


# ---- 3. the table's own invariants -------------------------------------------------------------------------------------------
def test_the_table_states_every_kind_once():
    with open(os.path.join(ROOT, "include", "aware_hip.h")) as f:
        header = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"^#define AWARE_LOOP_([A-Z_]+) (\d+)\b", f.read(), re.M)}
    n = len(LA.TABLE)            # twelve today; a later kind adds a row, and nothing here pins the count
    assert n >= 12 and [k.id for k in LA.TABLE] == list(range(n))
    assert {k.name: k.id for k in LA.TABLE} == header == LA.KINDS
    assert list(LA.KINDS)[:12] == NAMES and list(LA.KINDS.values()) == list(range(n))
    assert LA.SPLITTING == tuple(k.name for k in LA.TABLE if k.splits) and LA.SPLITTING[:9] == tuple(NAMES[2:8] + NAMES[9:])
    for k in LA.TABLE:
        assert callable(k.parse) and callable(k.device) and callable(k.apply), k.name
        assert k.check is None or callable(k.check), k.name
        assert "kind" in k.keys and "prob" in k.keys and k.display
        assert LA.kind_id(k.name) == k.id
    assert LA.kind_id("chorus") is None and LA.kind_id(3) is None and LA.kind_id(None) is None
    # the C table: the same numbers, the same splitting kinds, kinds 2 to 11 for the _ex entry points only, and the splitting
    # kinds alone ranked where a refused chain is sized
    with open(os.path.join(ROOT, "aware_amd", "csrc", "loop_limits.hpp")) as f:
        limits = f.read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bkLoop([A-Za-z]+) = (\d+)", limits)}
    camel = lambda name: "".join(w.capitalize() for w in name.split("_"))
    assert {name: ids[camel(name)] for name in LA.KINDS} == LA.KINDS
    rows = [(m.group(1) == "true", m.group(2) == "true", int(m.group(3)), int(m.group(4)))
            for m in re.finditer(r"^\s*\{(true|false), (true|false), (-?\d+)\},\s*//\s*(\d+) ", limits, re.M)]
    assert [r[3] for r in rows] == list(range(n))
    assert [r[0] for r in rows] == [k.splits for k in LA.TABLE] and [r[1] for r in rows] == [k.id >= 2 for k in LA.TABLE]
    assert sorted(r[2] for r in rows if r[0]) == list(range(len(LA.SPLITTING))) and all(r[2] == -1 for r in rows if not r[0])
