"""The streaming STFT / iSTFT kernels (csrc/dsp_stream.hip, csrc/fft512.hpp) keep their bits when a value moves to another
place in LDS or travels by another LDS instruction: the exchange layouts, the twiddle / window / merge tables and the mel rows
carry no arithmetic, so every result of the streaming path is the same bit pattern before and after such a change.

Batches:
  ragged    [513, 4096, 12000] samples: a one-frame-of-signal clip (3 frames), a clip shorter than one run (17 frames) and a
            clip of several runs whose last run is partial (47 frames)
  uniform   64 x 16000: the short run length (4 frames per analysis run, 4 hop blocks per synthesis run)

Arrays, per batch (card band 32..256, mel fold on, use_graph False):
  mag, U    aware_stft_band (the exact decomposition of the original audio: analysis<AN_NORM, POLAR>)
  rec       aware_istft of aware_stft of the batch
  y         the raw synthesis of the third forward pass (buffer 9: synth<SY_FWD>)
  g0, g3    aware_embed_gradient before the first and after the third step: it passes through the mel rows of
            analysis<AN_NORM, MELF>, the detector, the expanded mel gradients of synth<SY_ADJ, MELG> (gy) and analysis<AN_ADJ>.
            The mel rows and gy themselves are not among the buffers the C API hands out: a changed bit in either changes g.
  coef      the coefficients after three fused optimiser steps, and best_coef, loss, pred

(a) against the workgroup-staged kernels (dsp_path "staged") with the bounds of test_gpu_kernels.test_stream_vs_staged_dsp_kernels:
    first loss and prediction 5e-6, first gradient rel L2 2e-4 (5e-2 for clips below 8 frames: two or three pooled frames, an
    ill-conditioned InstanceNorm), loss after three steps 2e-3 and output 2e-2 on clips of 8 frames or more.  rec against the
    audio it came from: 1e-5 absolute (the clips are 0.1 sigma noise, |x| < 0.6: a float32 transform pair of 10 radix-2 levels
    and a four-term overlap-add is a few 1e-7 away; 1e-5 leaves the usual factor for the envelope division at the clip ends).
(b) bit for bit against tests/golden/stream_parent_bits.json: the sha256 of the same arrays recorded on the MI355X with
    aware_amd/csrc/ of the parent commit ("Detectors with temporal convolutions: kernel_size, stride, padding"), by
    `python tests/test_gpu_stream_lds_bits.py OUT.json` there.  The fixture also holds the sha256 of each batch's inputs.

The wide-band (band 0..512) and L1 (push_extremes_l1) instantiations share the FFT helpers: once each on the ragged batch,
check (a) only (the L1 kernels its first-iteration part: test_l1_instantiations_against_staged says why).

Run on the MI355X box:  python -m pytest tests/test_gpu_stream_lds_bits.py -m gpu -q -s"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import GOLDEN, make_clip  # noqa: E402

pytestmark = pytest.mark.gpu

CARD = (32, 256)
BATCHES = {"ragged": [513, 4096, 12000], "uniform": [16000] * 64}
SEED0 = {"ragged": 300, "uniform": 320}
FIXTURE = os.path.join(GOLDEN, "stream_parent_bits.json")
BIT_ARRAYS = ["mag", "U", "rec", "y", "g0", "g3", "coef", "best_coef", "loss", "pred"]


@pytest.fixture(scope="module")
def rt():
    from aware_amd import runtime
    from aware_amd._lib import require_gpu
    require_gpu()
    return runtime


@pytest.fixture(scope="module")
def O():
    from oracle import aware_oracle
    return aware_oracle


def inputs(O, bname):
    lengths = BATCHES[bname]
    pairs = [make_clip(SEED0[bname] + i, n) for i, n in enumerate(lengths)]
    wm = np.stack([O.bits_to_bipolar(p[1]) for p in pairs]).astype(np.float32)
    return [p[0] for p in pairs], wm


_PLANS, _DETS = {}, {}


def plan_det(rt, O, band):
    if band not in _PLANS:
        _PLANS[band] = rt.Plan(band_bins=band)
        ws, bs = O.detector_weights()
        _DETS[band] = rt.DetectorWeights(_PLANS[band], O.mel_filter_bank(), [w.numpy() for w in ws], [b.numpy() for b in bs])
    return _PLANS[band], _DETS[band]


_RUNS = {}


def run(rt, O, bname, dsp_path, band=CARD, **kw):
    """Every array of the header for one batch and one DSP path, on the host, computed once."""
    key = (bname, dsp_path, band, tuple(sorted(kw.items())))
    if key in _RUNS:
        return _RUNS[key]
    clips, wm = inputs(O, bname)
    plan, det = plan_det(rt, O, band)
    batch = rt.Batch(BATCHES[bname])
    audio = batch.pack(clips)
    r = {"batch": batch}
    if dsp_path == "stream":
        r["mag"], r["U"] = rt.stft_band(plan, batch, audio, normalize=True)
        r["rec"] = rt.istft(plan, batch, rt.stft(plan, batch, audio))
    sess = rt.EmbedSession(plan, det, batch, use_graph=False, dsp_path=dsp_path, num_iterations=8, **kw)
    sess.begin(audio, torch.from_numpy(wm).cuda())
    r["g0"] = sess.gradient().clone()
    r["loss0"], r["pred0"] = sess.loss.clone(), sess.pred.clone()
    sess.iterate(3)
    r["coef"], r["best_coef"] = sess.coef.clone(), sess.best_coef.clone()
    r["loss"], r["pred"] = sess.loss.clone(), sess.pred.clone()
    r["g3"] = sess.gradient().clone()
    r["y"] = sess._view(9, (batch.total_out,)).clone()
    r["out"] = sess.finish(None).clone()
    torch.cuda.synchronize()
    r = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in r.items()}
    _RUNS[key] = r
    return r


def sha(t):
    a = t.numpy() if torch.is_tensor(t) else np.asarray(t)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digests(rt, O):
    out = {"inputs": {}, "sha256": {}}
    for bname in BATCHES:
        clips, wm = inputs(O, bname)
        out["inputs"][bname] = sha(np.concatenate(clips + [wm.ravel()]))
        r = run(rt, O, bname, "stream")
        out["sha256"][bname] = {k: sha(r[k]) for k in BIT_ARRAYS}
    return out


def check_against_staged(r1, r0, tag, after_steps=True):
    """(a) of the header: r1 the streaming path, r0 the staged one; after_steps False: the first iteration only."""
    batch = r1["batch"]
    for k in ("g0", "g3", "coef", "y", "out", "loss", "pred"):
        assert bool(torch.isfinite(r1[k]).all()), (tag, k)
    dl, dp = float((r1["loss0"] - r0["loss0"]).abs().max()), float((r1["pred0"] - r0["pred0"]).abs().max())
    print(f"{tag}: first loss difference {dl:.2e}, prediction {dp:.2e}")
    assert dl < 5e-6 and dp < 5e-6, (tag, dl, dp)
    ok = np.asarray([t >= 8 for t in batch.frames])
    for i in range(batch.B if batch.B <= 4 else 4):
        sl = slice(batch.frame_offsets[i], batch.frame_offsets[i + 1])
        g1, g0 = r1["g0"][sl].double(), r0["g0"][sl].double()
        if float(g0.norm()) == 0.0:                                # a single pooled frame: zero variance, zero gradient
            assert float(g1.abs().max()) == 0.0, (tag, i)
            continue
        rel = float((g1 - g0).norm() / g0.norm())
        print(f"{tag} clip {i} ({batch.frames[i]} frames): stream vs staged first gradient rel L2 {rel:.2e}")
        assert rel < (2e-4 if batch.frames[i] >= 8 else 5e-2), (tag, i, rel)
    if not after_steps:
        return
    dl3 = float(np.max(np.abs((r1["loss"] - r0["loss"]).numpy())[ok]))
    print(f"{tag}: loss difference after three steps {dl3:.2e}")
    assert dl3 < 2e-3, (tag, dl3)
    for i in np.nonzero(ok)[0]:
        sl = slice(batch.out_offsets[i], batch.out_offsets[i] + batch.out_lengths[i])
        do = float((r1["out"][sl] - r0["out"][sl]).abs().max())
        assert do < 2e-2, (tag, int(i), do)


@pytest.mark.parametrize("bname", list(BATCHES))
def test_stream_against_staged(rt, O, bname):
    r1, r0 = run(rt, O, bname, "stream"), run(rt, O, bname, "staged")
    check_against_staged(r1, r0, bname)
    batch = r1["batch"]
    clips, _ = inputs(O, bname)
    for i, c in enumerate(clips):
        n = batch.out_lengths[i]
        err = float((r1["rec"][batch.out_offsets[i]: batch.out_offsets[i] + n] - torch.from_numpy(c[:n])).abs().max())
        assert err < 1e-5, (bname, i, err)
    nb = CARD[1] - CARD[0] + 1
    assert float(r1["mag"][:, nb:].abs().max()) == 0.0 and float(r1["mag"].max()) > 0.0
    assert float((r1["coef"] - r1["mag"]).abs().max()) > 0.0        # the three steps moved the coefficients


@pytest.mark.parametrize("bname", list(BATCHES))
def test_stream_keeps_the_parent_bits(rt, O, bname):
    with open(FIXTURE) as f:
        want = json.load(f)
    clips, wm = inputs(O, bname)
    assert sha(np.concatenate(clips + [wm.ravel()])) == want["inputs"][bname], "the inputs differ, not the kernels"
    r = run(rt, O, bname, "stream")
    assert sorted(want["sha256"][bname]) == sorted(BIT_ARRAYS)
    bad = [k for k in BIT_ARRAYS if sha(r[k]) != want["sha256"][bname][k]]
    assert not bad, (bname, bad)


def test_wide_instantiations_against_staged(rt, O):
    r1, r0 = run(rt, O, "ragged", "stream", (0, 512)), run(rt, O, "ragged", "staged", (0, 512))
    check_against_staged(r1, r0, "wide")


def test_l1_instantiations_against_staged(rt, O):
    """The staged kernels have no L1 form (aware_embed_create refuses push_extremes_l1 with dsp_path "staged"), so the L1
    kernels are held against the staged plain loss where the two objectives agree: at c = c0 the L1 term and its gradient
    (sign(0) = 0) are exactly zero, so the first loss, prediction and gradient obey the same bounds.  After three steps the
    objectives differ by design: there the L1 session is finite, and away from the plain session's coefficients (the L1
    kernels, not the plain ones, ran)."""
    r1 = run(rt, O, "ragged", "stream", CARD, loss="push_extremes_l1", l1_weight=0.5)
    check_against_staged(r1, run(rt, O, "ragged", "staged"), "l1", after_steps=False)
    assert float((r1["coef"] - run(rt, O, "ragged", "stream")["coef"]).abs().max()) > 0.0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from aware_amd import runtime
    from oracle import aware_oracle
    with open(sys.argv[1], "w") as f:
        json.dump(digests(runtime, aware_oracle), f, indent=0, sort_keys=True)
    print("wrote", sys.argv[1])
