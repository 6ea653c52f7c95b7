#!/usr/bin/env python3
"""Generate tests/golden/wide_band.npz by running the reference on the CPU at embedding bands of the wide layout.

TEST INFRASTRUCTURE, like tools/make_golden.py (same import recipe and stand-ins, imported from it): it runs only where the
reference tree exists and writes data only.  Contents, per band B in {0_8000, 300_7000} (Hz; bins 0..512 and 20..448):

  net/B/{pred, grad}: the model card's AWAREDetectorNet on seeded magnitudes [2, 513, 63] that are zero outside the band,
      one clip per call; pred [2, 20, 1] and the in-band magnitude gradient of each clip's push_extremes loss against
      `target`, every GRAD_STEP-th frame.
  traj/B/{losses, out_sample, out_step, out_len, raw_marked, det_bits}: the reference's own 400-step embed of the 1 s seed
      clip (make_golden's seed 1) with the model card's embedding_bands edited to B (built as the reference's load() builds
      it); the waveform every OUT_STEP-th sample.
  Subsampled so that the file stays small.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_wide_band.py
"""
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _setup_import_path, make_clip  # noqa: E402

MAG_SEED = 91
MAG_SHAPE = (2, 513, 63)
GRAD_STEP = 8
OUT_STEP = 4
BANDS_HZ = ((0, 8000), (300, 7000))


def band_bins(hz):
    f = np.linspace(0, 8000, 513)
    idx = np.where((f >= hz[0]) & (f <= hz[1]))[0]
    return int(idx[0]), int(idx[-1])


def magnitudes(lo, hi):
    """Seeded band-limited magnitudes: |complex Gaussian| in bins lo..hi, zero elsewhere (the detector's input)."""
    rng = np.random.default_rng(MAG_SEED)
    m = np.zeros(MAG_SHAPE, np.float32)
    z = rng.standard_normal((MAG_SHAPE[0], hi - lo + 1, MAG_SHAPE[2], 2))
    m[:, lo:hi + 1, :] = (0.3 * np.hypot(z[..., 0], z[..., 1])).astype(np.float32)
    return m


def key(hz):
    return f"{hz[0]}_{hz[1]}"


def main():
    _setup_import_path()
    import matplotlib
    matplotlib.use("Agg")
    from aware.detection.multibit_detector_net import AWAREDetectorNet
    from aware.embedding.losses import PushToExtremesLoss
    from aware.embedding import AWAREEmbedder
    from aware.detection import AWAREDetector
    from aware.service import embed_watermark, detect_watermark

    def build(cfg):
        """The reference's load() (utils/models/load_model.py:6-76) on an edited card: it only reads its own file."""
        shared = {k: cfg.get(k, v) for k, v in (("frame_length", 1024), ("hop_length", 256), ("window", "hann"),
                                                ("win_length", 1024))}
        bands = tuple(cfg.get("embedding_bands", [500, 4000]))
        emb = AWAREEmbedder(pattern_mode=cfg.get("pattern_mode", "bits2bipolar"), embedding_bands=bands,
                            tolerance_db=cfg.get("tolerance_db", 6.0), num_iterations=cfg.get("num_iterations", 400),
                            detection_net_cfg=cfg.get("detection_net_cfg", {}), optimizer_cfg=cfg.get("optimizer_cfg"),
                            scheduler_cfg=cfg.get("scheduler_cfg"), loss=cfg.get("loss", "push_extremes"),
                            verbose=cfg.get("verbose", True), **shared)
        det = AWAREDetector(model=emb.detection_net, threshold=cfg.get("threshold", 0.0),
                            pattern_mode=cfg.get("pattern_mode", "bipolar"), embedding_bands=bands, **shared)
        return emb, det

    torch.set_num_threads(8)
    d = {"mag_seed": MAG_SEED, "mag_shape": np.asarray(MAG_SHAPE), "grad_step": GRAD_STEP}
    rng = np.random.default_rng(MAG_SEED + 1)
    target = torch.from_numpy(np.where(rng.integers(0, 2, (2, 20, 1)) > 0, 1.0, -1.0).astype(np.float32))
    d["target"] = target.numpy()
    net = AWAREDetectorNet().eval()
    for p in net.parameters():
        p.requires_grad = False
    for hz in BANDS_HZ:
        lo, hi = band_bins(hz)
        mag0 = torch.from_numpy(magnitudes(lo, hi))
        preds, grads = [], []
        for b in range(MAG_SHAPE[0]):
            mag = mag0[b:b + 1].clone().requires_grad_(True)
            pred = net(mag)
            PushToExtremesLoss()(pred, target[b:b + 1]).backward()
            preds.append(pred.detach().numpy()[0])
            grads.append(mag.grad.numpy()[0, lo:hi + 1, ::GRAD_STEP].copy())
        d[f"net/{key(hz)}/pred"] = np.stack(preds)
        d[f"net/{key(hz)}/grad"] = np.stack(grads)
        print(key(hz), d[f"net/{key(hz)}/pred"][0, :4, 0])

    card = yaml.safe_load(open(os.path.join(REF, "src", "AWARE", "cards", "config.yaml")))
    audio, bits = make_clip(1, 16000)
    for hz in BANDS_HZ:
        cfg = dict(card)
        cfg["embedding_bands"] = list(hz)
        embedder, detector = build(cfg)
        losses = []
        orig = embedder.loss

        class _Rec:
            def __call__(self, p, t):
                v = orig(p, t)
                losses.append(float(v.detach()))
                return v

        embedder.loss = _Rec()
        wm_audio = embed_watermark(audio, 16000, bits, embedder)
        embedder.loss = orig
        k = f"traj/{key(hz)}"
        d[k + "/losses"] = np.asarray(losses, np.float64)
        d[k + "/out_len"] = wm_audio.shape[0]
        d[k + "/out_step"] = OUT_STEP
        d[k + "/out_sample"] = wm_audio[::OUT_STEP].astype(np.float32)
        d[k + "/raw_marked"] = detector.detect(wm_audio, 16000).astype(np.float32)
        d[k + "/det_bits"] = np.asarray(detect_watermark(wm_audio, 16000, detector))
        print(k, "loss0", losses[0], "best", min(losses), "bits", bits.tolist(), "det", d[k + "/det_bits"].tolist())
    np.savez_compressed(os.path.join(OUT, "wide_band.npz"), **d)
    print("written", os.path.abspath(os.path.join(OUT, "wide_band.npz")))


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("reference tree not present: this script only runs in the development container")
    main()
