"""The phase vocoder inside the embed loop (EXTENSION): the torch restatement (aware_amd/embedding/loop_attacks.py: pv_draw,
pv_frames, pv_stretch, apply_chain) against the oracle's phase vocoder, the two kernels' order written out in numpy against the
restatement and against autograd, the draws and the chains the entry may not stand in, the card keys, the C ABI's symbols, and
the value claim on the CPU -- what the vocoder inside the loop buys against the oracle's time stretch and pitch shift, through
the oracle's embed loop.  No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, make_clip
from oracle import aware_oracle as O
from aware_amd.embedding import loop_attacks as LA
from test_loop_attacks_host import AttackedEmbedder, ber, unit_clip
from test_loop_speed_host import snr_db

PV_RATE = {"kind": "phase_vocoder", "rate": [0.85, 1.15]}
PV_CENTS = {"kind": "phase_vocoder", "cents": 150.0}
PV_BOTH = {"kind": "phase_vocoder", "rate": [0.85, 1.15], "cents": 150.0}
PITCH = {"kind": "pitch_shift", "cents": 100.0}
SPEED = {"kind": "speed_change", "cents": 100.0}
STRETCH = {"kind": "time_stretch", "rate": 1.15}
NOISE10 = {"kind": "gaussian_noise", "snr_db": 10.0}
SUP = {"kind": "sample_suppression", "seconds": 0.3}
REVERB = {"kind": "reverberation", "rt60": 0.3}
Q_MIN, Q_MAX = -16384, 21845                               # the stretch's range of offsets
M_MIN, M_MAX = -13520, 17034                               # the speed offsets of -+400 cents


def spectrum(T, seed=0, F=513):
    """A seeded complex spectrum [T, F] with a zero frame, zero cells and real DC / Nyquist columns."""
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((T, F)) + 1j * rng.standard_normal((T, F))
    S[:, 0], S[:, -1] = S[:, 0].real, S[:, -1].real
    S[min(7, T - 1)] = 0
    S[min(3, T - 1), 5] = S[0, 9] = S[T - 1, 11] = 0
    return S


def kernel_order(S, mq, G=None):
    """csrc/loop_pv_kernels.hip line by line, all bins at once, in float64: S[i] and S[i + 1] as (|c|, u(c), live) in registers,
    the two frames behind them in flight, P advanced and renormalised per frame.  G None: Y.  Otherwise gS from G = dL/dY, gmag[i]
    and gmag[i + 1] in registers, a row flushed when i leaves it."""
    T, F = S.shape
    if mq == 0:
        return (S if G is None else G).copy()

    def load(r):
        return S[r].copy() if r < T else np.zeros(F, dtype=complex)

    def cell(c):
        s = np.maximum(np.abs(c.real), np.abs(c.imag))
        z = s == 0
        sd = np.where(z, 1.0, s)
        xs, ys = c.real / sd, c.imag / sd
        h = np.where(z, 1.0, np.sqrt(xs * xs + ys * ys))
        return np.where(z, 0.0, s * h), np.where(z, 1.0, xs / h) + 1j * (ys / h), np.where(z, 0.0, 1.0)

    Q = 65536 + mq
    out = np.full((T, F), np.nan + 0j)
    i, c0, c1, n0, n1 = 0, cell(load(0)), cell(load(1)), load(2), load(3)
    P = c0[1].copy()
    g0, g1 = np.zeros(F), np.zeros(F)
    for t in range(T):
        p = t * Q
        it = p >> 16
        if it >= T:
            if G is not None:
                break
            out[t] = 0
            continue
        assert it - i <= 2
        while i < it:
            if G is not None:
                out[i] = g0 * c0[1] * c0[2]
                g0, g1 = g1, np.zeros(F)
            c0, c1, n0, n1 = c1, cell(n0), n1, load(i + 4)
            i += 1
        al = (p & 0xFFFF) / 65536.0
        if G is not None:
            gm = P.real * G[t].real + P.imag * G[t].imag
            g0, g1 = g0 + (1 - al) * gm, g1 + al * gm
        else:
            out[t] = (al * c1[0] + (1 - al) * c0[0]) * P
        P = P * (c1[1] * np.conj(c0[1]))
        P = P * (1.5 - 0.5 * np.abs(P) ** 2)
    if G is not None:
        out[i] = g0 * c0[1] * c0[2]
        if i + 1 < T:
            out[i + 1] = g1 * c1[1] * c1[2]
        out[i + 2:] = 0
    assert not np.isnan(out).any()
    return out


# ---- 1. the model -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [17, 40])
@pytest.mark.parametrize("Q", [49152, 65535, 65537, 87381, 70000])
def test_product_form_is_the_oracles_phase_vocoder(T, Q):
    """P is the textbook accumulator: on the first min(T, ceil(T / rate)) frames the restatement equals oracle.phase_vocoder at
    rate = Q / 65536.  Both compute in float64; the oracle returns complex64, so the bound is that format's rounding of each
    value (2^-24 per part) and a few float64 ulps of the accumulated phase, which the restatement multiplies and the oracle adds."""
    S = spectrum(T)
    rate = Q / 65536.0
    n = min(T, math.ceil(T / rate))
    Y = LA.pv_frames(torch.from_numpy(S), Q - 65536).numpy()
    ref = O.phase_vocoder(S.T, rate).T.astype(np.complex128)
    assert Y.shape == (T, 513) and ref.shape[0] >= n
    err = np.abs(Y[:n] - ref[:n])
    print(f"Q = {Q}, T = {T}: largest difference {err.max():.3e} on {n} frames, peak {np.abs(ref[:n]).max():.3f}")
    assert np.all(err <= 2.0 ** -23 * np.abs(ref[:n]) + 1e-12)
    i, al, live = LA.pv_positions(T, Q - 65536)
    assert np.all(Y[~live] == 0) and np.array_equal(live, np.arange(T) * Q < (T << 16))
    assert np.all(np.diff(i) <= 2) and np.all(np.diff(i) >= 0)               # monotone, 0, 1 or 2 per frame


@pytest.mark.parametrize("mq", [Q_MIN, Q_MAX, -1, 1, 4464])
def test_kernel_order_is_the_restatement(mq):
    """The register window of the kernel (two cells held, two frames in flight, rows loaded once) computes the restatement; the
    per-frame Newton step on |P| changes nothing at float64."""
    for T in (1, 2, 3, 17, 32):
        S = spectrum(T, seed=T)
        Y = LA.pv_frames(torch.from_numpy(S), mq).numpy()
        err = np.abs(kernel_order(S, mq) - Y).max()
        assert err <= 1e-12, (T, mq, err)


def test_identity():
    S = torch.from_numpy(spectrum(9))
    assert LA.pv_frames(S, 0) is S and np.array_equal(kernel_order(S.numpy(), 0), S.numpy())
    x = unit_clip(2, 4099)
    assert LA.pv_stretch(x, 0) is x
    assert LA.pv_stretch(x, 300).shape == x.shape and LA.pv_stretch(x.float(), 300).dtype == torch.float32
    z = LA.apply_chain(x[None], [{"kind": "phase_vocoder", "rate": [1.0, 1.0], "cents": [0.0, 0.0]}], [3], 0)
    np.testing.assert_array_equal(z.numpy(), x[None].numpy())


def peak_hz(z, sr=16000):
    spec = np.abs(np.fft.rfft(z * np.hanning(len(z))))
    k = int(np.argmax(spec))
    a, b, c = np.log(spec[k - 1: k + 2])
    return (k + 0.5 * (a - c) / (a - 2 * b + c)) * sr / len(z)


def test_a_sine_keeps_its_frequency_when_stretched_and_moves_in_pitch_mode():
    """A 1 kHz sine stretched at 1.1 stays at 1 kHz and ends in zeros after Ny / 1.1; in pitch mode it moves by the interval at
    its duration."""
    n = 16128
    x = torch.sin(2 * np.pi * 1000.0 * torch.arange(n, dtype=torch.float64) / 16000)
    mq = 6554                                                                 # 1.1
    y = LA.pv_stretch(x, mq).numpy()
    assert abs(peak_hz(y[2048:10240]) - 1000.0) < 1.0
    i, _, live = LA.pv_positions(n // 256 + 1, mq)
    dead = int(np.argmin(live))                                               # the first output frame past the end of the clip
    assert abs(256 * dead - n / 1.1) < 512
    assert np.all(y[256 * dead + 256:] == 0) and np.abs(y[256 * dead - 1536: 256 * dead - 512]).max() > 0.9
    for cents in (-100.0, 150.0):
        e = LA.parse_chain([{"kind": "phase_vocoder", "cents": [cents, cents + 0.1]}])[0]
        mq, m = LA.pv_draw(e, LA.entry_draw(0, 0, 0))
        assert mq == LA.pitch_offsets(m)[1] - 65536 and abs(1200 * math.log2((65536 + m) / 65536) - cents) < 0.2
        z = LA.apply_chain(x[None], [e], [0], 0)[0].numpy()
        np.testing.assert_array_equal(z, LA.speed_change(LA.pv_stretch(x, mq), m).numpy())
        assert abs(peak_hz(z[2048:10240]) - 1000.0 * (65536 + m) / 65536) < 1.0
        # downwards the clip lasts as long as it did; upwards the lengthened intermediate was cut at Ny, so the resampled clip
        # ends at Ny 65536 / R and in zeros (the model keeps every signal on the clip's own Ny samples)
        end = min(n, n * 65536 // (65536 + m))
        # (without phase locking the bins beside the sine's drift against it: the textbook vocoder's loss of amplitude)
        assert np.abs(z[end - 3000: end - 1500]).max() > 0.5 and np.all(z[end + 1024:] == 0)


# ---- 2. the backward pass ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mq", [Q_MIN, Q_MAX, -1, 1, 4464])
def test_backward_in_the_kernels_order_is_autograd(mq):
    """gm[t] = Re(conj(P[t]) G[t]), the two taps transposed onto the input frames over ascending t, gS[i] = gmag[i] u(S[i]) and 0
    at a zero cell: within 1e-12 of autograd on the float64 restatement, for the frames alone and through both transforms."""
    for T in (2, 17, 32):
        Sn = spectrum(T, seed=10 + T)
        G = spectrum(T, seed=20 + T) + 0.3
        S = torch.from_numpy(Sn).requires_grad_(True)
        Y = LA.pv_frames(S, mq)
        (Y.real * torch.from_numpy(G.real) + Y.imag * torch.from_numpy(G.imag)).sum().backward()
        gs = kernel_order(Sn, mq, G)
        err = np.abs(gs - S.grad.numpy()).max()
        assert err <= 1e-12, (T, mq, err)
        assert np.all(gs[Sn == 0] == 0)
    n = 4099
    x = unit_clip(5, n).requires_grad_(True)
    w = torch.from_numpy(np.cos(0.37 * np.arange(n)) * np.linspace(0.2, 1.0, n))
    (LA.pv_stretch(x, mq) * w).sum().backward()
    x2 = unit_clip(5, n).requires_grad_(True)
    S = LA._loop_stft(x2)
    Yl = S.detach().clone().requires_grad_(True)                             # a leaf in Y's place: the iSTFT adjoint alone
    (LA._loop_istft(Yl) * w[:4096]).sum().backward()
    gS = torch.from_numpy(kernel_order(S.detach().numpy(), mq, Yl.grad.numpy()))
    S.backward(gS)                                                           # the STFT adjoint
    err = float((x2.grad - x.grad).abs().max())
    assert err <= 1e-12 * max(1.0, float(x.grad.abs().max())), (mq, err)


# ---- 3. draws and chain rules -----------------------------------------------------------------------------------------------------
def test_draws_differ_and_both_modes_occur():
    e = {k: LA.parse_chain([c])[0] for k, c in (("rate", PV_RATE), ("cents", PV_CENTS), ("both", PV_BOTH))}
    draws = {k: [LA.pv_draw(e[k], LA.entry_draw(sd, s, 0)) for sd in range(4) for s in range(16)] for k in e}
    assert all(m == 0 and -9831 <= mq <= 9830 for mq, m in draws["rate"])
    assert all(m != 0 and mq == LA.pitch_offsets(m)[1] - 65536 and Q_MIN <= mq <= Q_MAX for mq, m in draws["cents"])
    assert len(set(draws["rate"])) >= 60 and len(set(draws["cents"])) >= 60
    stretch = [d for d in draws["both"] if d[1] == 0]
    assert 16 <= len(stretch) <= 48                                           # even odds: 32 +- 4 sigma of 64 draws
    for (sd, s), d in zip([(sd, s) for sd in range(4) for s in range(16)], draws["both"]):
        r = LA.entry_draw(sd, s, 0)
        assert d == (draws["rate"][sd * 16 + s] if int(r[2]) < 2 ** 31 else draws["cents"][sd * 16 + s])
    x = torch.stack([unit_clip(1, 4096), unit_clip(1, 4096)])
    z0, z1 = LA.apply_chain(x, [PV_BOTH], [0, 1], 0), LA.apply_chain(x, [PV_BOTH], [0, 1], 1)
    assert float((z0[0] - z0[1]).abs().max()) > 0.05 and float((z0[0] - z1[0]).abs().max()) > 0.05
    np.testing.assert_array_equal(LA.apply_chain(x, [PV_BOTH], [0, 1], 0).numpy(), z0.numpy())
    mq, m = draws["both"][16]                                                 # seed 1, step 0
    np.testing.assert_array_equal(z0[1].numpy(), LA.speed_change(LA.pv_stretch(x[1], mq), m).numpy())


def test_probability():
    x = unit_clip(4, 2048)[None]
    for step in range(5):
        np.testing.assert_array_equal(LA.apply_chain(x, [dict(PV_BOTH, prob=0.0)], [9], step).numpy(), x.numpy())
    assert all(not torch.equal(LA.apply_chain(x, [dict(PV_BOTH, prob=1.0)], [9], s), x) for s in range(5))
    fired = sum(int(LA.fires(LA.entry_draw(2, s, 0)[0], 0.75)) for s in range(400))
    assert 0.68 * 400 < fired < 0.82 * 400, fired                             # 0.75 +- 3 sigma of 400 draws
    for s in range(12):
        on = LA.fires(LA.entry_draw(2, s, 0)[0], 0.75)
        assert torch.equal(LA.apply_chain(x, [dict(PV_RATE, prob=0.75)], [2], s), x) == (not on)


def test_order_with_noise_and_suppression_and_ragged_lists():
    n = 7936
    x = unit_clip(6, n)[None]
    e = LA.parse_chain([PV_BOTH])[0]
    mq, m = LA.pv_draw(e, LA.entry_draw(1, 0, 0))
    res = LA.apply_chain(x, [e], [1], 0)[0]
    np.testing.assert_array_equal(res.numpy(), LA.speed_change(LA.pv_stretch(x[0], mq), m).numpy())
    both = LA.apply_chain(x, [e, NOISE10], [1], 0)[0]                         # noise behind: sigma from the vocoded signal
    sigma = np.sqrt(float((res ** 2).mean()) / 10.0)
    np.testing.assert_allclose((both - res).numpy(), sigma * LA.normal_draws(n, 1, 0, 1), atol=1e-12)
    front = LA.apply_chain(x, [NOISE10, e], [1], 0)[0]                        # noise in front: it is vocoded too, by entry 1's draw
    noisy = LA.apply_chain(x, [NOISE10], [1], 0)[0]
    mq1, m1 = LA.pv_draw(e, LA.entry_draw(1, 0, 1))
    np.testing.assert_array_equal(front.numpy(), LA.speed_change(LA.pv_stretch(noisy, mq1), m1).numpy())
    sup = {"kind": "sample_suppression", "seconds": 0.1}
    b = LA.apply_chain(x, [e, sup], [1], 0)[0]
    s_b = LA.suppression_start(LA.entry_draw(1, 0, 1)[1], n, 1600)
    assert float(b[s_b:s_b + 1600].abs().max()) == 0.0
    assert LA.apply_chain(x, [sup, NOISE10, e, NOISE10], [1], 3).shape == x.shape
    clips = [unit_clip(1, 4099), unit_clip(2, 7937)]
    out = LA.apply_chain(clips, [PV_BOTH], [4, 5], 2)
    assert isinstance(out, list) and [len(o) for o in out] == [4099, 7937]
    np.testing.assert_array_equal(out[1].numpy(), LA.apply_chain(clips[1][None], [PV_BOTH], [5], 2)[0].numpy())
    assert np.all(LA.pv_stretch(clips[1], -3000).numpy()[7936:] == 0)         # past the iSTFT's 256 (n // 256) samples


@pytest.mark.parametrize("chain", [
    [{"kind": "phase_vocoder"}],
    [{"kind": "phase_vocoder", "prob": 0.5}],
    [{"kind": "phase_vocoder", "rate": 1.0}],
    [{"kind": "phase_vocoder", "rate": 0.9}],
    [{"kind": "phase_vocoder", "rate": 1.4}],
    [{"kind": "phase_vocoder", "rate": [1.1, 0.9]}],
    [{"kind": "phase_vocoder", "rate": [0.7, 1.0]}],
    [{"kind": "phase_vocoder", "rate": [1.0, 1.34]}],
    [{"kind": "phase_vocoder", "rate": [0.9, 1.0, 1.1]}],
    [{"kind": "phase_vocoder", "rate": float("nan")}],
    [{"kind": "phase_vocoder", "rate": [0.9, float("inf")]}],
    [{"kind": "phase_vocoder", "rate": "fast"}],
    [{"kind": "phase_vocoder", "rate": [1.000001, 1.000002]}],                            # no offset inside
    [{"kind": "phase_vocoder", "cents": 0.0}],
    [{"kind": "phase_vocoder", "cents": -50.0}],
    [{"kind": "phase_vocoder", "cents": [50.0, -50.0]}],
    [{"kind": "phase_vocoder", "cents": 400.5}],
    [{"kind": "phase_vocoder", "cents": [-401.0, 0.0]}],
    [{"kind": "phase_vocoder", "cents": float("nan")}],
    [{"kind": "phase_vocoder", "cents": [-10.0, 0.0, 10.0]}],
    [{"kind": "phase_vocoder", "cents": "high"}],
    [{"kind": "phase_vocoder", "cents": [0.001, 0.002]}],                                 # no speed offset inside
    [{"kind": "phase_vocoder", "rate": 1.1, "cents": 500.0}],                             # one good key does not excuse the other
    [{"kind": "phase_vocoder", "rate": 1.5, "cents": 100.0}],
    [{"kind": "phase_vocoder", "rate": 1.1, "prob": 1.5}],
    [{"kind": "phase_vocoder", "rate": 1.1, "prob": -0.1}],
    [{"kind": "phase_vocoder", "rate": 1.1, "rt60": 0.3}],
    [{"kind": "phase_vocoder", "cents": 100.0, "seconds": 0.3}],
    [PV_RATE, PV_CENTS], [PV_BOTH, NOISE10, PV_BOTH],
    [PV_BOTH, REVERB], [REVERB, PV_BOTH], [REVERB, NOISE10, PV_RATE], [PV_CENTS, SUP, REVERB],
    [PV_BOTH, SPEED], [SPEED, PV_BOTH], [SPEED, NOISE10, PV_RATE], [PV_CENTS, NOISE10, SPEED],
    [PV_BOTH, STRETCH], [STRETCH, PV_BOTH], [STRETCH, NOISE10, PV_RATE], [PV_CENTS, SUP, STRETCH],
    [PV_BOTH, PITCH], [PITCH, PV_BOTH], [PITCH, NOISE10, PV_RATE], [PV_CENTS, SUP, PITCH],
    [STRETCH, SPEED, PV_BOTH], [PV_BOTH, STRETCH, SPEED],
    [PV_BOTH, NOISE10, SUP, NOISE10, SUP],
])
def test_invalid_chains_are_refused(chain):
    with pytest.raises(ValueError):
        LA.parse_chain(chain)
    from aware_amd.embedding import AWAREEmbedder
    with pytest.raises(ValueError):
        AWAREEmbedder(loss="push_extremes", verbose=False, loop_attacks=chain)


# ---- 4. surface and pins ----------------------------------------------------------------------------------------------------------
def test_parse_and_device_entries():
    assert LA.KINDS["phase_vocoder"] == 6 and LA.KINDS["pitch_shift"] == 5
    c = LA.parse_chain([{"kind": "sample_suppression", "seconds": 0.5}, {"kind": "phase_vocoder", "rate": 1.25, "cents": 100},
                        {"kind": "gaussian_noise", "snr_db": 10}])
    assert c[1] == {"kind": "phase_vocoder", "prob": 1.0, "rate": [0.8, 1.25], "cents": [-100.0, 100.0]}
    assert LA.parse_chain(c) == c                                                          # a parsed chain parses to itself
    assert LA.device_entries_ex(c, 16000) == [(1, 1.0, [8000.0, 0.0, 0.0, 0.0]), (6, 1.0, [-13107.0, 16384.0, -3678.0, 3896.0]),
                                              (0, 1.0, [10.0, 0.0, 0.0, 0.0])]
    r = LA.parse_chain([dict(PV_RATE, prob=0.75)])
    assert r == [{"kind": "phase_vocoder", "prob": 0.75, "rate": [0.85, 1.15]}]
    assert LA.device_entries_ex(r, 16000) == [(6, 0.75, [-9830.0, 9830.0, 0.0, -1.0])]    # an absent mode: lo > hi
    assert LA.stretch_range(r[0]) == LA.stretch_range(LA.parse_chain([{"kind": "time_stretch", "rate": [0.85, 1.15]}])[0])
    ct = LA.parse_chain([{"kind": "phase_vocoder", "cents": (-50.0, 120.0)}])
    m_lo, m_hi = LA.speed_range(LA.parse_chain([{"kind": "speed_change", "cents": [-50.0, 120.0]}])[0])
    assert LA.device_entries_ex(ct, 16000) == [(6, 1.0, [0.0, -1.0, float(m_lo), float(m_hi)])]
    full = LA.parse_chain([{"kind": "phase_vocoder", "rate": [0.75, 4.0 / 3.0], "cents": 400.0}])
    assert LA.device_entries_ex(full, 16000) == [(6, 1.0, [float(Q_MIN), float(Q_MAX), float(M_MIN), float(M_MAX)])]
    mq = [LA.pitch_offsets(m)[1] - 65536 for m in (M_MIN, M_MAX)]
    assert Q_MIN <= min(mq) and max(mq) <= Q_MAX                                           # the coupled rate stays inside
    # chains of the older kinds say what they said
    old = LA.parse_chain([{"kind": "time_stretch", "rate": 1.25}, {"kind": "speed_change", "cents": 100}])
    assert LA.device_entries_ex(old, 16000) == [(4, 1.0, [-13107.0, 16384.0, 0.0, 0.0]), (3, 1.0, [-3678.0, 3896.0, 0.0, 0.0])]
    assert LA.device_entries_ex(LA.parse_chain([PITCH]), 16000) == [(5, 1.0, [-3678.0, 3896.0, 0.0, 0.0])]


def test_card_keys_reach_the_embedder(tmp_path):
    from aware_amd.utils.models import load
    with open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")) as f:
        text = f.read()
    assert "# loop_attacks: [{kind: phase_vocoder, rate: [0.85, 1.15], cents: 150.0, prob: 0.9}]" in text
    card = yaml.safe_load(text)
    card["loop_attacks"] = yaml.safe_load("[{kind: gaussian_noise, snr_db: 20.0}, {kind: phase_vocoder, rate: [0.85, 1.15], cents: 150.0, prob: 0.9}]")
    card["loop_attack_seed"] = 5
    p = tmp_path / "card.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    assert emb.loop_attacks == [{"kind": "gaussian_noise", "prob": 1.0, "snr_db": 20.0},
                                {"kind": "phase_vocoder", "prob": 0.9, "rate": [0.85, 1.15], "cents": [-150.0, 150.0]}]
    assert emb.loop_attack_seed == 5
    card["loop_attacks"] = [PV_BOTH, SPEED]
    p.write_text(yaml.safe_dump(card))
    assert load(str(p)) is None


def test_abi_symbols_and_bad_arguments():
    from aware_amd import _lib
    lib = _lib.load_library()
    for name in ("aware_pv_frames", "aware_pv_frames_bwd"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "loop_pv_kernels.hip" in _lib.SOURCES
    assert lib.aware_version() == 350
    assert C.sizeof(_lib.LoopAttackEx) == 24 and C.sizeof(_lib.LoopAttack) == 12
    with open(os.path.join(ROOT, "include", "aware_hip.h")) as f:
        hdr = f.read()
    assert "#define AWARE_LOOP_PHASE_VOCODER 6" in hdr and "int aware_pv_frames(" in hdr and "int aware_pv_frames_bwd(" in hdr
    ent = (_lib.LoopAttackEx * 1)(_lib.LoopAttackEx(6, 0.9, (C.c_float * 4)(-9830.0, 9830.0, -5435.0, 5930.0)))
    seeds = (C.c_uint32 * 1)(0)
    assert lib.aware_embed_set_loop_attacks_ex(None, ent, 1, seeds, None, 0, None) == -1
    assert lib.aware_embed_loop_attack_workspace_bytes_ex(None, ent, 1) == 0
    old = (_lib.LoopAttack * 1)(_lib.LoopAttack(6, 0.0, 1.0))                               # kind 6 through the older call
    assert lib.aware_embed_set_loop_attacks(None, old, 1, seeds, None, 0, None) == -1
    # the stand-alone entries refuse null pointers, sizes out of range and buffers that may not coincide before any launch
    p, q, g = C.c_void_p(256), C.c_void_p(512), C.c_void_p(768)                             # never dereferenced
    for hole in range(4):
        args = [p, p, 1, p, q]
        args[hole + (hole >= 2)] = None
        assert lib.aware_pv_frames(*args, None) == -1
    for B in (0, -1, 65536):
        assert lib.aware_pv_frames(p, p, B, p, q, None) == -1
    assert lib.aware_pv_frames(p, p, 1, p, p, None) == -1                                   # out == spec
    for hole in range(5):
        args = [p, g, p, 1, p, q]
        args[hole + (hole >= 3)] = None
        assert lib.aware_pv_frames_bwd(*args, None) == -1
    for B in (0, -1, 65536):
        assert lib.aware_pv_frames_bwd(p, g, p, B, p, q, None) == -1
    assert lib.aware_pv_frames_bwd(p, g, p, 1, p, g, None) == -1                            # grad_spec == grad_out


def test_no_new_attack_class():
    from aware_amd import attacks as A
    assert not any("vocoder" in k.lower() for k in A.ATTACKS)
    assert "TimeStretch" in A.ATTACKS and "PitchShift" in A.ATTACKS


# ---- 5. the value claim, on the CPU -----------------------------------------------------------------------------------------------
CHAINS = {"stretch-aware": [dict(PV_RATE, prob=0.75)], "pitch-aware": [dict(PV_CENTS, prob=0.75)], "both": [dict(PV_BOTH, prob=0.9)]}
RATES = [0.9, 0.95, 1.05, 1.1]
CENTS = [-100, -50, 50, 100]


def test_phase_vocoder_in_the_loop_against_the_oracles_attacks():
    """Four 1 s clips, 400 steps, card settings: plain, and the phase vocoder inside the loop in stretch mode (rate 0.85 to 1.15,
    prob 0.75), in pitch mode (+-150 cents, prob 0.75) and with both keys (prob 0.9), against the oracle's phase-vocoder pitch
    shift at -+50 and -+100 cents and its time stretch at 0.9, 0.95, 1.05 and 1.1.  The bounds: clean 0 %; the plain means at
    least 25 % (pitch) and 10 % (stretch), so that there is something to win; the stretch-aware stretch mean at most half the
    plain one (the ratio of test_loop_attacks_host.py), the pitch-aware pitch mean at most two thirds of the plain one (DESIGN.md
    section 18's threshold); the embedding with both keys meets both.  Measured figures: DESIGN.md section 20."""
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    pairs = [make_clip(s, 16000) for s in range(4)]
    audio = np.stack([p[0] for p in pairs])
    bits = np.stack([p[1] for p in pairs])
    wm = np.stack([O.bits_to_bipolar(b) for b in bits]).astype(np.float32)
    plain = O.Embedder()
    ys = {"plain": plain.embed(audio, wm)[0].numpy()}
    for k, chain in CHAINS.items():
        ys[k] = AttackedEmbedder(chain, [0, 1, 2, 3]).embed(audio, wm)[0].numpy()
    names = list(ys)
    clean = {k: ber(plain, bits, y) for k, y in ys.items()}
    print("clean BER: " + " / ".join(f"{k} {clean[k]:.2f} %" for k in names))
    ps = {k: [ber(plain, bits, np.stack([O.pitch_shift_attack(c.astype(np.float32), ct) for c in ys[k]])) for ct in CENTS] for k in names}
    for i, c in enumerate(CENTS):
        print(f"pitch shift by {c:+d} cents: " + " / ".join(f"{k} {ps[k][i]:.2f} %" for k in names))
    st = {k: [ber(plain, bits, np.stack([O.time_stretch_attack(c.astype(np.float32), r) for c in ys[k]])) for r in RATES] for k in names}
    for i, r in enumerate(RATES):
        print(f"phase vocoder stretch at {r}: " + " / ".join(f"{k} {st[k][i]:.2f} %" for k in names))
    mp = {k: float(np.mean(ps[k])) for k in names}
    ms = {k: float(np.mean(st[k])) for k in names}
    print("mean over the four pitch shifts: " + " / ".join(f"{k} {mp[k]:.2f} %" for k in names))
    print("mean over the four rates: " + " / ".join(f"{k} {ms[k]:.2f} %" for k in names))
    for k in names:
        print(f"SNR against the normalised host, dB, {k}: " + ", ".join(f"{v:.2f}" for v in snr_db(ys[k], audio)))
    assert all(clean[k] == 0.0 for k in names)
    assert mp["plain"] >= 25.0 and ms["plain"] >= 10.0
    assert ms["stretch-aware"] <= 0.5 * ms["plain"]
    assert mp["pitch-aware"] <= 2.0 / 3.0 * mp["plain"]
    assert ms["both"] <= 0.5 * ms["plain"] and mp["both"] <= 2.0 / 3.0 * mp["plain"]
