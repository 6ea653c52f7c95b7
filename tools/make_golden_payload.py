#!/usr/bin/env python3
"""Generate tests/golden/payload_lengths.npz by running the reference's detector at other payload lengths on the CPU.

TEST INFRASTRUCTURE, like tools/make_golden_variants.py (same import recipe and stand-ins, imported from tools/make_golden.py):
it runs only where the reference tree exists and writes data only.  Contents:

  net/L<L>/{pred, grad, target}: AWAREDetectorNet(output_length=L) on make_golden_variants' seeded band-limited magnitudes
      [2, 513, 63] (bins outside 32..256 zero), one clip per call; pred [2, L, 1] and the band magnitude gradient of each
      clip's push_extremes loss against a seeded bipolar `target` [2, L, 1], every GRAD_STEP-th frame ([2, 225, 8]),
      for L in LENGTHS.
  traj/L64/{bits, losses, out_sample, out_step, out_len, raw_marked, det_bits}: the reference's own 400-step embed of the
      1 s seed clip (make_golden's seed 1) with a 64-bit payload (seeded bits) and an edited model card (watermark_length
      and detection_net_cfg.output_length 64, built as the reference's load() builds it); the waveform every OUT_STEP-th
      sample.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_payload.py
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
from make_golden_variants import GRAD_STEP, MAG_SEED, MAG_SHAPE, OUT_STEP, magnitudes  # noqa: E402

LENGTHS = (1, 21, 33, 64, 128, 512)
TRAJ_L = 64
BITS_SEED = 640


def targets(L):
    rng = np.random.default_rng(MAG_SEED + L)
    return np.where(rng.integers(0, 2, (MAG_SHAPE[0], L, 1)) > 0, 1.0, -1.0).astype(np.float32)


def traj_bits():
    return np.random.default_rng(BITS_SEED).integers(0, 2, TRAJ_L).astype(np.int32)


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
    d = {"mag_seed": MAG_SEED, "mag_shape": np.asarray(MAG_SHAPE), "grad_step": GRAD_STEP, "lengths": np.asarray(LENGTHS)}
    mag0 = torch.from_numpy(magnitudes())
    for L in LENGTHS:
        net = AWAREDetectorNet(output_length=L).eval()
        for p in net.parameters():
            p.requires_grad = False
        target = torch.from_numpy(targets(L))
        preds, grads = [], []
        for b in range(MAG_SHAPE[0]):
            mag = mag0[b:b + 1].clone().requires_grad_(True)
            pred = net(mag)
            PushToExtremesLoss()(pred, target[b:b + 1]).backward()
            preds.append(pred.detach().numpy()[0])
            grads.append(mag.grad.numpy()[0, 32:257, ::GRAD_STEP].copy())
        key = f"net/L{L}"
        d[key + "/pred"] = np.stack(preds)
        d[key + "/grad"] = np.stack(grads)
        d[key + "/target"] = target.numpy()
        print(key, d[key + "/pred"][0, :4, 0])

    card = yaml.safe_load(open(os.path.join(REF, "src", "AWARE", "cards", "config.yaml")))
    audio, _ = make_clip(1, 16000)
    bits = traj_bits()
    cfg = dict(card)
    cfg["watermark_length"] = TRAJ_L
    cfg["detection_net_cfg"] = dict(card["detection_net_cfg"], output_length=TRAJ_L)
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
    key = f"traj/L{TRAJ_L}"
    d[key + "/bits"] = bits
    d[key + "/losses"] = np.asarray(losses, np.float64)
    d[key + "/out_len"] = wm_audio.shape[0]
    d[key + "/out_step"] = OUT_STEP
    d[key + "/out_sample"] = wm_audio[::OUT_STEP].astype(np.float32)
    d[key + "/raw_marked"] = detector.detect(wm_audio, 16000).astype(np.float32)
    d[key + "/det_bits"] = np.asarray(detect_watermark(wm_audio, 16000, detector))
    print(key, "loss0", losses[0], "best", min(losses), "bits", bits.tolist(), "det", d[key + "/det_bits"].tolist())
    np.savez_compressed(os.path.join(OUT, "payload_lengths.npz"), **d)
    print("written", os.path.abspath(os.path.join(OUT, "payload_lengths.npz")))


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("reference tree not present: this script only runs in the development container")
    main()
