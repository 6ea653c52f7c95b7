"""Host-side checks of the wide band layout (no GPU): the band -> stride rule, the C ABI's new entry point and version."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_band_stride_rule():
    from aware_amd import runtime as rt
    from aware_amd.utils.audio.plugins import band_bins
    assert rt.SPEC_STRIDE == 256 and rt.SPEC_STRIDE_WIDE == 576
    assert rt.SPEC_STRIDE_WIDE % 64 == 0 and rt.SPEC_STRIDE_WIDE >= 513      # 9 bins per lane; K % 64 for the mel GEMMs
    # the model card's band and every band the narrow layout took before keep it
    assert band_bins(16000, 1024, (500, 4000)) == (32, 256)
    for lo, hi in [(32, 256), (1, 256), (1, 1), (256, 511), (511, 511), (300, 511), (100, 355)]:
        assert rt.band_stride(lo, hi) == 256, (lo, hi)
    # the issue's edits: wider than 256 bins, or touching DC / Nyquist
    for hz, bins in [((300, 7000), (20, 448)), ((1000, 6000), (64, 384)), ((0, 8000), (0, 512))]:
        assert band_bins(16000, 1024, hz) == bins
        assert rt.band_stride(*bins) == 576, hz
    for lo, hi in [(0, 0), (0, 256), (512, 512), (256, 512), (1, 511), (100, 356)]:
        assert rt.band_stride(lo, hi) == 576, (lo, hi)
    with pytest.raises(ValueError):
        band_bins(16000, 1024, (7000, 300))          # an empty band keeps its ValueError


def test_header_declares_band_stride():
    with open(os.path.join(ROOT, "include", "aware_hip.h")) as f:
        h = f.read()
    assert re.search(r"int aware_plan_band_stride\(const aware_plan\* plan\);", h)
    assert re.search(r"#define AWARE_SPEC_STRIDE 256\b", h)
    assert re.search(r"#define AWARE_SPEC_STRIDE_WIDE 576\b", h)
    with open(os.path.join(ROOT, "aware_amd", "csrc", "common.hpp")) as f:
        c = f.read()
    assert "constexpr int kFS = 256;" in c and "constexpr int kFSWide = 576;" in c


def test_library_exports_band_stride():
    from aware_amd._lib import SIGNATURES, load_library
    lib = load_library()
    assert "aware_plan_band_stride" in SIGNATURES
    assert hasattr(lib, "aware_plan_band_stride")
    assert lib.aware_version() >= 330
    assert lib.aware_plan_band_stride(None) < 0        # AWARE_E_BADARG on a null plan, no GPU needed


GOLDEN = os.path.join(ROOT, "tests", "golden", "wide_band.npz")
GOLDEN_BANDS = {"0_8000": (0, 512), "300_7000": (20, 448)}


def golden_magnitudes(lo, hi, seed=91, shape=(2, 513, 63)):
    """tools/make_golden_wide_band.py magnitudes(): |complex Gaussian| in bins lo..hi, zero elsewhere."""
    import numpy as np
    rng = np.random.default_rng(seed)
    m = np.zeros(shape, np.float32)
    z = rng.standard_normal((shape[0], hi - lo + 1, shape[2], 2))
    m[:, lo:hi + 1, :] = (0.3 * np.hypot(z[..., 0], z[..., 1])).astype(np.float32)
    return m


def wide_embedder(O, bins, **kw):
    """The oracle's embed loop with its band replaced by bins lo..hi (the reference's mask on linspace(0, 8000, 513))."""
    e = O.Embedder(**kw)
    e.band, e.nonband = O.band_indices(bands=(bins[0] * 15.625, bins[1] * 15.625))
    assert e.band[0] == bins[0] and e.band[-1] == bins[1]
    return e


@pytest.mark.parametrize("band", list(GOLDEN_BANDS))
def test_float64_detector_vs_reference_golden(band):
    """The oracle's detector in float64 on the golden's band-limited magnitudes: the reference's predictions and in-band
    magnitude gradients (push_extremes) at a band of the wide layout."""
    import numpy as np
    import torch
    from oracle import aware_oracle as O
    fx = np.load(GOLDEN)
    lo, hi = GOLDEN_BANDS[band]
    det = O.Detector(torch.float64)
    mag = torch.from_numpy(golden_magnitudes(lo, hi)).double().requires_grad_(True)
    tg = torch.from_numpy(fx["target"]).double()
    preds = []
    for b in range(2):
        pred = det.forward(mag[b:b + 1])
        p, t = pred.reshape(1, -1), tg[b].reshape(1, -1)
        (((p - t) ** 2).mean() - 0.1 * p.abs().mean()).backward()
        preds.append(pred.detach().numpy()[0])
    np.testing.assert_allclose(np.stack(preds).reshape(2, -1), fx[f"net/{band}/pred"].reshape(2, -1), atol=2e-5)
    step = int(fx["grad_step"])
    g = mag.grad.numpy()[:, lo:hi + 1, ::step]
    ref = fx[f"net/{band}/grad"]
    for b in range(2):
        assert np.linalg.norm(g[b] - ref[b]) / np.linalg.norm(ref[b]) < 1e-4, (band, b)


@pytest.mark.parametrize("band", list(GOLDEN_BANDS))
def test_float64_loop_vs_reference_trajectory(band):
    """A float64 restatement of the embed loop (oracle, band replaced) against the reference's 400-step embed of the 1 s seed
    clip at a band of the wide layout: loss within 1.6e-2 at every step, waveform within 0.15 relative L2, bits equal."""
    import numpy as np
    import torch
    from conftest import make_clip
    from oracle import aware_oracle as O
    fx = np.load(GOLDEN)
    emb = wide_embedder(O, GOLDEN_BANDS[band], dtype=torch.float64)
    audio, bits = make_clip(1, 16000)
    wm = O.bits_to_bipolar(bits).astype(np.float64)[None]
    losses = []
    y, _ = emb.embed(audio.astype(np.float64)[None], wm, record=lambda it, l, p, g: losses.append(float(l[0])))
    ref = fx[f"traj/{band}/losses"]
    d = np.abs(np.asarray(losses) - ref)
    assert d[0] < 1e-5 and d.max() <= 1.6e-2, (band, d[0], d.max())
    out = (y[0].numpy() * float(np.max(audio))).astype(np.float32)
    assert out.shape[0] == int(fx[f"traj/{band}/out_len"])
    r = fx[f"traj/{band}/out_sample"]
    assert np.linalg.norm(out[::int(fx[f"traj/{band}/out_step"])] - r) / np.linalg.norm(r) <= 0.15
    raw = emb.detect_raw(out[None].astype(np.float64))[0].numpy()
    np.testing.assert_array_equal(O.decode_bits(raw), fx[f"traj/{band}/det_bits"])
