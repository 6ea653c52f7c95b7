"""The host images of a detector's parameters (no device): csrc/detector_image.hpp -- the storage rule, the check of a create
call's arguments, the padded f32 image, the two sparse mel forms, the packed operands' layouts and the BatchNorm image -- through
tests/host_sim/detector_image_check.cpp against a numpy restatement of the header's comments.  Every comparison is exact: the
images are copies and zero fills.  All values are distinct integers, so that a swapped index cannot pass."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from aware_amd import runtime as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, TAPS_A, TAPS_B = 256, 6, 12           # kFS, kMelTapsA, kMelTapsB (csrc/common.hpp)
OK, BADARG, UNSUPPORTED = 0, -1, -2
CARD_BAND = (32, 225, 256, 512, 0)        # lo, nband, stride, n_fft, general: a band behind bin 0 and narrower than its row


def detector_image_check():
    """tests/host_sim/detector_image_check.cpp, built without HIP where it is missing or older than its sources.  Returns
    run(lines) -> one dict per line."""
    exe = os.path.join(ROOT, "tests", "host_sim", "detector_image_check")
    src = os.path.join(ROOT, "tests", "host_sim", "detector_image_check.cpp")
    hdrs = [os.path.join(ROOT, "aware_amd", "csrc", "detector_image.hpp"), os.path.join(ROOT, "include", "aware_hip.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in [src] + hdrs):
        cxx = ["g++", "-O2", "-std=c++17"] if shutil.which("g++") else ["hipcc", "-O2", "-std=c++17", "-x", "hip", "--offload-host-only"]
        subprocess.run(cxx + ["-o", exe, src], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(line + "\n" for line in lines), check=True, capture_output=True, text=True).stdout
        got = [json.loads(line) for line in out.splitlines()]
        assert len(got) == len(lines)
        return got

    return run


def spec_tokens(channels, n_mels=None, n_layers=None, conv=(1, 1, 0), pool=(2, 2)):
    ch = list(channels or [])
    return [ch[0] if n_mels is None else n_mels, len(ch) - 1 if n_layers is None else n_layers, len(ch)] + ch + list(conv) + list(pool)


# ---- the storage rule ------------------------------------------------------------------------------------------------------
def test_storage_rule_is_the_python_rule():
    got = detector_image_check()(["stored"])[0]
    assert got["hidden"] == [rt.stored_channels([128, c, 64, 40])[1] for c in range(1, 4097)]
    assert got["last"] == [rt.stored_channels([128, 64, 64, c])[3] for c in range(2, 1025, 2)]


# ---- the check of a create call --------------------------------------------------------------------------------------------
def check_line(channels=(128, 256, 40), n_mels=None, n_layers=None, conv=(1, 1, 0), pool=(2, 2), required=1, arch=2, act=1, norm=0,
               final=4, pointers=1, plan=1):
    """arch 0: null, 1: null scale / shift arrays, 2: arrays, 3: arrays whose last entries are null."""
    return " ".join(map(str, ["check"] + spec_tokens(channels, n_mels, n_layers, conv, pool) + [required, arch, act, norm, final, pointers, plan]))


# (arguments, the code the chain aware_detector_create_pool -> _conv -> _ex -> detector_create returned), in the order of the checks
CHECKS = [
    (dict(), OK),
    (dict(required=0, arch=0), OK),                                    # aware_detector_create
    (dict(conv=(7, 4, 3), pool=(8, 8)), OK), (dict(conv=(3, 1, 1), pool=(2, 3)), OK),
    (dict(channels=[512, 4096, 1024]), OK), (dict(channels=[128] + [8] * 32 + [2]), OK),
    (dict(norm=1), OK),
    # the pool: arguments, then support
    (dict(pool=(0, 2)), BADARG), (dict(pool=(2, 0)), BADARG), (dict(pool=(-1, -1)), BADARG),
    (dict(pool=(9, 2)), UNSUPPORTED), (dict(pool=(2, 9)), UNSUPPORTED), (dict(pool=(1, 2)), UNSUPPORTED), (dict(pool=(2, 1)), UNSUPPORTED),
    # the convolution: arguments, then support
    (dict(conv=(0, 1, 0)), BADARG), (dict(conv=(1, 0, 0)), BADARG), (dict(conv=(1, 1, -1)), BADARG),
    (dict(conv=(8, 1, 0)), UNSUPPORTED), (dict(conv=(3, 5, 0)), UNSUPPORTED), (dict(conv=(3, 1, 2)), UNSUPPORTED),
    (dict(conv=(1, 1, 1)), UNSUPPORTED),                               # kernel 1 / stride 1 takes padding 0 only
    (dict(conv=(1, 2, 1)), UNSUPPORTED),
    # the architecture: null on the _ex, _conv and _pool paths, enum ranges, the BatchNorm arrays
    (dict(arch=0), BADARG), (dict(arch=0, conv=(3, 1, 1)), BADARG), (dict(arch=0, conv=(3, 1, 1), pool=(4, 4)), BADARG),
    (dict(arch=0, pool=(4, 4)), BADARG),
    (dict(act=-1), BADARG), (dict(act=4), BADARG), (dict(norm=-1), BADARG), (dict(norm=3), BADARG), (dict(final=-1), BADARG),
    (dict(final=6), BADARG), (dict(act=3, norm=2, final=5), OK),
    (dict(norm=1, arch=1), BADARG), (dict(norm=1, arch=3), BADARG), (dict(norm=0, arch=1), OK),
    (dict(norm=1, n_layers=0), BADARG), (dict(norm=1, n_layers=34), BADARG),      # BatchNorm counts its blocks before the sizes do
    # the pointers
    (dict(pointers=0), BADARG), (dict(channels=None, n_mels=128, n_layers=2), BADARG),
    # the plan
    (dict(plan=0), UNSUPPORTED),
    # the sizes
    (dict(n_mels=0), UNSUPPORTED), (dict(channels=[513, 64, 40]), UNSUPPORTED), (dict(n_layers=0), UNSUPPORTED),
    (dict(n_layers=34), UNSUPPORTED), (dict(n_mels=64), UNSUPPORTED), (dict(channels=[128, 256, 41]), UNSUPPORTED),
    (dict(channels=[128, 256, 0]), UNSUPPORTED), (dict(channels=[128, 256, 1026]), UNSUPPORTED),
    (dict(channels=[128, 0, 40]), UNSUPPORTED), (dict(channels=[128, 64, 4097, 40]), UNSUPPORTED),
    # wrong in two ways: the earlier code
    (dict(pool=(0, 2), conv=(8, 1, 0)), BADARG), (dict(pool=(9, 2), conv=(0, 1, 0)), UNSUPPORTED),
    (dict(pool=(2, 2), conv=(0, 1, 0)), BADARG), (dict(pool=(2, 2), conv=(8, 1, 0)), UNSUPPORTED),
    (dict(pool=(4, 4), conv=(0, 1, 0)), BADARG), (dict(pool=(4, 4), conv=(8, 1, 0), arch=0), UNSUPPORTED),
    (dict(conv=(8, 1, 0), arch=0), UNSUPPORTED), (dict(arch=0, plan=0), BADARG), (dict(arch=0, n_mels=0), BADARG),
    (dict(pointers=0, plan=0), BADARG), (dict(plan=0, channels=None, n_mels=128, n_layers=2), BADARG),
    (dict(required=0, arch=0, plan=0, n_mels=0), UNSUPPORTED),
]


def test_create_checks_return_the_chain_s_codes():
    got = detector_image_check()([check_line(**kw) for kw, _ in CHECKS])
    assert [(kw, g["rc"]) for (kw, _), g in zip(CHECKS, got)] == [(kw, rc) for kw, rc in CHECKS]


# ---- the images ------------------------------------------------------------------------------------------------------------
def make_case(channels, conv=(1, 1, 0), pool=(2, 2), band=CARD_BAND, bias_mask=None, mel=None):
    """A detector's arguments with all-distinct integer values.  bias_mask: -1 = no biases at all, else bit l = biases[l] given
    (default: all)."""
    nl, K = len(channels) - 1, conv[0]
    nbins = band[3] // 2 + 1
    at = [1]

    def take(shape):
        n = int(np.prod(shape))
        v = np.arange(at[0], at[0] + n, dtype=np.float32).reshape(shape)
        at[0] += n
        return v

    weights = [take((channels[l + 1], channels[l], K)) for l in range(nl)]
    biases = [take((channels[l + 1],)) for l in range(nl)]
    mel = take((channels[0], nbins)) if mel is None else np.asarray(mel, dtype=np.float32)
    assert at[0] < 2 ** 24 and mel.shape == (channels[0], nbins)
    return dict(channels=list(channels), conv=conv, pool=pool, band=band, bias_mask=(1 << nl) - 1 if bias_mask is None else bias_mask,
                mel=mel, weights=weights, biases=biases)


def image_line(c):
    nums = spec_tokens(c["channels"], conv=c["conv"], pool=c["pool"]) + list(c["band"]) + [c["bias_mask"]]
    data = np.concatenate([c["mel"].ravel()] + [w.ravel() for w in c["weights"]] + [b.ravel() for b in c["biases"]]).astype(np.int64)
    return "image " + " ".join(map(str, nums)) + " " + " ".join(map(str, data.tolist()))


def expected_image(c):
    """detector_image.hpp's comment on DetectorImage, in numpy: the parts in order, and the flat image."""
    ch, st = c["channels"], rt.stored_channels(c["channels"])
    K = c["conv"][0]
    lo, nband, S = c["band"][:3]
    melT = np.zeros((st[0], S), np.float32)
    melT[:ch[0], :nband] = c["mel"][:, lo:lo + nband]
    parts = {"melT": melT, "melB": melT.T}
    for l in range(len(ch) - 1):
        w = np.zeros((st[l + 1], K, st[l]), np.float32)                      # column j * ci + c = tap j of input channel c
        w[:ch[l + 1], :, :ch[l]] = c["weights"][l].transpose(0, 2, 1)
        w = w.reshape(st[l + 1], K * st[l])
        b = np.zeros(st[l + 1], np.float32)
        if c["bias_mask"] >= 0 and c["bias_mask"] >> l & 1:
            b[:ch[l + 1]] = c["biases"][l]
        parts.update({f"w{l}": w, f"wT{l}": w.T, f"b{l}": b})
    return parts, np.concatenate([p.ravel() for p in parts.values()])


def part_offsets(parts):
    off, at = {}, 0
    for k, p in parts.items():
        off[k] = at
        at += p.size
    return off


# channel lists: every boundary padded (16, 32, 16); hidden and last above 64 (128, 128); nothing padded; temporal convolutions
# on a padded input width (the tap-major column); no biases; one block without a bias; a band of a general geometry
IMAGE_CASES = {
    "padded": make_case([13, 30, 14]),
    "above64": make_case([8, 65, 66]),
    "card": make_case([128, 256, 40]),
    "taps": make_case([12, 6, 4], conv=(3, 1, 1)),
    "no_biases": make_case([13, 30, 14], bias_mask=-1),
    "one_bias_null": make_case([13, 30, 14], bias_mask=0b01),
    "short_band": make_case([12, 6, 4], band=(3, 100, 136, 256, 1)),
    "mixed": make_case([128, 256, 64, 40]),
    "taps128": make_case([128, 128, 40], conv=(3, 1, 1)),
    "pooled": make_case([128, 128, 40], pool=(4, 4)),
    "one_layer": make_case([128, 40]),
}


@pytest.fixture(scope="module")
def images():
    got = detector_image_check()([image_line(c) for c in IMAGE_CASES.values()])
    return dict(zip(IMAGE_CASES, got))


@pytest.mark.parametrize("name", list(IMAGE_CASES))
def test_f32_image(images, name):
    c, g = IMAGE_CASES[name], images[name]
    parts, flat = expected_image(c)
    off = part_offsets(parts)
    nl = len(c["channels"]) - 1
    assert (g["o_melT"], g["o_melB"]) == (off["melT"], off["melB"])
    assert g["o_w"] == [off[f"w{l}"] for l in range(nl)] and g["o_wT"] == [off[f"wT{l}"] for l in range(nl)]
    assert g["o_b"] == [off[f"b{l}"] for l in range(nl)]
    h = np.asarray(g["h"], np.float32)
    assert h.shape == flat.shape and np.array_equal(h, flat)
    # what the image promises, on the program's own output
    ch, st = c["channels"], rt.stored_channels(c["channels"])
    K, (lo, nband, S) = c["conv"][0], c["band"][:3]
    melT = h[g["o_melT"]:g["o_melT"] + st[0] * S].reshape(st[0], S)
    melB = h[g["o_melB"]:g["o_melB"] + st[0] * S].reshape(S, st[0])
    assert np.array_equal(melB, melT.T) and not melT[ch[0]:].any() and not melT[:, nband:].any()
    assert np.array_equal(melT[:ch[0], :nband], c["mel"][:, lo:lo + nband])
    for l in range(nl):
        ci, co = st[l], st[l + 1]
        w = h[g["o_w"][l]:g["o_w"][l] + K * ci * co].reshape(co, K, ci)
        wT = h[g["o_wT"][l]:g["o_wT"][l] + K * ci * co].reshape(K * ci, co)
        assert np.array_equal(wT, w.reshape(co, K * ci).T)
        assert not w[ch[l + 1]:].any() and not w[:, :, ch[l]:].any() and w[:ch[l + 1], :, :ch[l]].all()
        b = h[g["o_b"][l]:g["o_b"][l] + co]
        assert not b[ch[l + 1]:].any() and b[:ch[l + 1]].all() == (c["bias_mask"] >= 0 and bool(c["bias_mask"] >> l & 1))
    assert not g["sparse"] and not g["runs"]              # a dense basis


# ---- the packed operands: the stand-ins of detector_image_check.cpp for the GEMM files' rules ----
def x3_bytes(N, K): return 6 * N * K + 6
def h2_bytes(N, K): return 4 * N * K + 4 * N + 4
def h2_ok(N, K): return N % 128 == 0 and K % 64 == 0
def readout_ok(ci, C): return ci % 128 == 0 and C <= 48


def expected_slots(c):
    """(bf16x3 slots, f16 slots) as (name, on, N, K), in the order of the allocation."""
    st = rt.stored_channels(c["channels"])
    nl, K, S = len(st) - 1, c["conv"][0], c["band"][2]
    fused = c["conv"] == (1, 1, 0) and c["pool"] == (2, 2)
    x3, h2 = [], []
    for l in range(nl):
        ci, co = K * st[l], st[l + 1]
        x3 += [(f"w{l}", co % 128 == 0 and ci % 64 == 0, co, ci), (f"wT{l}", ci % 128 == 0 and co % 64 == 0, ci, co)]
        h2 += [(f"w{l}", fused and h2_ok(st[l + 1], st[l]), st[l + 1], st[l]), (f"wT{l}", fused and h2_ok(st[l], st[l + 1]), st[l], st[l + 1])]
    ro = fused and nl >= 2 and readout_ok(st[nl - 1], st[nl])
    colp = -(-st[nl] // 16) * 16
    x3 += [("melT", st[0] % 128 == 0, st[0], S), ("melB", st[0] % 64 == 0, S, st[0]), ("last", ro, colp, st[nl - 1]), ("lastT", ro, st[nl - 1], 64)]
    return x3, h2


def got_slots(g, prefix, nl, tail):
    out = []
    for l in range(nl):
        out += [(f"w{l}", g[f"{prefix}_w"][l]), (f"wT{l}", g[f"{prefix}_wT"][l])]
    return out + [(k, g[f"{prefix}_{k}"]) for k in tail]


@pytest.mark.parametrize("name", list(IMAGE_CASES))
def test_packed_layouts(images, name):
    c, g = IMAGE_CASES[name], images[name]
    st = rt.stored_channels(c["channels"])
    nl = len(st) - 1
    for want, got, total, nbytes, align in (
            (expected_slots(c)[0], got_slots(g, "x3", nl, ["melT", "melB", "last", "lastT"]), g["x3_total"], x3_bytes, 1),
            (expected_slots(c)[1], got_slots(g, "h2", nl, []), g["h2_total"], h2_bytes, 256)):
        at = 0
        for (wname, on, N, K), (gname, (gon, goff, gN, gK)) in zip(want, got):
            assert (wname, int(on), N, K) == (gname, gon, gN, gK), (name, wname)
            assert goff == at, (name, wname)               # consecutive, so disjoint, in the order of the allocation
            if on:
                at += -(-nbytes(N, K) // align) * align
        assert total == at and len(want) == len(got)
    x3on = {k for k, on, _, _ in expected_slots(c)[0] if on}
    h2on = {k for k, on, _, _ in expected_slots(c)[1] if on}
    if name == "mixed":
        assert x3on == {"w0", "wT0", "wT1", "melT", "melB"} and h2on == {"w0", "wT0", "wT1"}
    if name in ("taps128", "pooled"):
        assert not {"last", "lastT"} & x3on and not h2on and g["h2_total"] == 0
    if name == "one_layer":
        assert not {"last", "lastT"} & x3on
    if name == "card":
        assert {"last", "lastT"} <= x3on
    # the read-out pair's re-padded operands
    if "last" in x3on:
        cil, col = st[nl - 1], st[nl]
        colp = -(-col // 16) * 16
        parts, _ = expected_image(c)
        want = np.zeros((colp, cil), np.float32)
        want[:col] = parts[f"w{nl - 1}"]
        wantT = np.zeros((cil, 64), np.float32)
        wantT[:, :col] = parts[f"w{nl - 1}"].T
        assert np.array_equal(np.asarray(g["last_rows"], np.float32).reshape(colp, cil), want)
        assert np.array_equal(np.asarray(g["lastT_rows"], np.float32).reshape(cil, 64), wantT)
        assert colp > col and want[:col].all()
    else:
        assert g["last_rows"] == [] and g["lastT_rows"] == []


# ---- the two mel forms -------------------------------------------------------------------------------------------------------
def bank(entries, n_mels=128, nbins=257):
    """A mel basis with the value 1 + its rank at each (filter, band column) of `entries` (the band starts at bin 1)."""
    m = np.zeros((n_mels, nbins), np.float32)
    for k, (j, f) in enumerate(entries):
        m[j, 1 + f] = k + 1
    return m


def triangular(n_mels=128):
    """Filter j on columns j, j + 1 -- column 128 holds the last filter alone; filter 5 is empty, and the columns from 129 on."""
    return [(j, f) for j in range(n_mels) if j != 5 for f in (j, j + 1)]


def lone(runs):
    """Filter j alone on the columns runs[j] = (first, length)."""
    return [(j, f) for j, (first, n) in runs.items() for f in range(first, first + n)]


MEL_BAND = (1, 256, 256, 512, 0)
MEL_CASES = {   # name: (entries, n_mels, band, sparse, runs)
    "triangular": (triangular(), 128, MEL_BAND, True, True),
    "late_filter": ([e for e in triangular() if e[0] != 127] + [(127, 250), (127, 251)], 128, MEL_BAND, True, True),   # start clamped to 244
    "late_filter_long": (lone({127: (246, 10), 3: (0, 2)}), 128, MEL_BAND, True, True),         # 244 + 12 columns just hold it
    "late_low_filter": (lone({20: (245, 6)}), 128, MEL_BAND, True, False),                      # ... 244 + 6 do not
    "three_in_a_column": (triangular() + [(42, 40)], 128, MEL_BAND, False, False),
    "two_not_adjacent": (lone({7: (30, 2), 9: (31, 2)}), 128, MEL_BAND, False, False),
    "low_filter_run_of_8": (lone({10: (20, 8), 70: (140, 2)}), 128, MEL_BAND, True, False),     # > kMelTapsA below filter 64
    "high_filter_run_of_8": (lone({70: (140, 8), 10: (20, 6)}), 128, MEL_BAND, True, True),     # <= kMelTapsB from 64 on
    "high_filter_run_of_13": (lone({70: (140, 13)}), 128, MEL_BAND, True, False),
    "bank_of_64": (triangular(64), 64, MEL_BAND, False, False),
    "general": (triangular(), 128, (1, 256, 256, 512, 1), False, False),
    "wide_stride": (triangular(), 128, (1, 256, 264, 512, 0), False, False),
}


def expected_forms(mel, band):
    """detector_image.hpp's comment on MelForms, in numpy (a basis that has both forms)."""
    lo, nband = band[:2]
    cols = mel[:, lo:lo + nband]
    tw, tm = np.zeros((FS, 2), np.float32), np.zeros(FS, np.int64)
    for f in range(nband):
        nz = np.flatnonzero(cols[:, f])
        if len(nz):
            tm[f] = min(nz[0], 126)
            tw[f] = cols[tm[f]:tm[f] + 2, f]
    fw, fs = np.zeros((128, TAPS_B), np.float32), np.zeros(128, np.int64)
    for j in range(128):
        nz = np.flatnonzero(cols[j])
        if len(nz):
            taps = TAPS_A if j < 64 else TAPS_B
            fs[j] = min(nz[0], FS - TAPS_B)
            fw[j, :taps] = np.pad(cols[j], (0, TAPS_B))[fs[j]:fs[j] + taps]
    return tw, tm, fw, fs


def test_mel_forms():
    cases = {k: make_case([n, 8, 4], band=band, mel=bank(e, n)) for k, (e, n, band, _, _) in MEL_CASES.items()}
    got = dict(zip(cases, detector_image_check()([image_line(c) for c in cases.values()])))
    for name, (_, _, band, sparse, runs) in MEL_CASES.items():
        g = got[name]
        assert (bool(g["sparse"]), bool(g["runs"])) == (sparse, runs), name
        if not sparse:
            continue
        tw, tm, fw, fs = expected_forms(cases[name]["mel"], band)
        assert np.array_equal(np.asarray(g["tw"], np.float32).reshape(FS, 2), tw), name
        assert g["tm"] == tm.tolist(), name
        if runs:
            assert np.array_equal(np.asarray(g["fw"], np.float32).reshape(128, TAPS_B), fw), name
            assert g["fs"] == fs.tolist(), name
    # what the cases are there for
    t = got["triangular"]
    assert t["tm"][128] == 126 and t["tw"][2 * 128] == 0 and t["tw"][2 * 128 + 1] != 0       # the last filter alone: the second tap
    assert t["tm"][5] == 4 and t["tw"][2 * 5 + 1] == 0 and t["tm"][6] == 6                    # around the empty filter
    assert t["tm"][129:] == [0] * 127 and not any(t["tw"][2 * 129:]) and t["fs"][5] == 0 and not any(t["fw"][5 * 12:6 * 12])
    late = got["late_filter"]
    assert late["fs"][127] == 244 and late["fw"][127 * 12:128 * 12] == [0] * 6 + late["tw"][2 * 250 + 1:2 * 252:2] + [0] * 4
    assert got["late_filter_long"]["fs"][127] == 244 and got["late_filter_long"]["fw"][127 * 12 + 11] != 0


# ---- the BatchNorm image -------------------------------------------------------------------------------------------------------
def test_norm_image():
    ch = [13, 30, 14]
    st = rt.stored_channels(ch)
    scale = [np.arange(1, 31), np.arange(31, 45)]
    shift = [np.arange(101, 131), np.arange(131, 145)]
    line = " ".join(map(str, ["norm"] + spec_tokens(ch) + np.concatenate(scale + shift).tolist()))
    g = detector_image_check()([line])[0]
    want, o_scale, o_shift = [], [], []
    for l in range(2):
        for o, v in ((o_scale, scale[l]), (o_shift, shift[l])):
            o.append(sum(len(x) for x in want))
            want.append(np.pad(v, (0, st[l + 1] - ch[l + 1])))
    assert g["h"] == np.concatenate(want).tolist() and g["n"] == 2 * (32 + 16)
    assert g["o_scale"] == o_scale and g["o_shift"] == o_shift
