#!/usr/bin/env python3
"""Generate tests/golden/detector_taps.npz by running the reference's detector with temporal convolutions on the CPU.

TEST INFRASTRUCTURE, like tools/make_golden_sizes.py (same import recipe and stand-ins, imported from tools/make_golden.py):
it runs only where the reference tree exists and writes data only.  Contents:

  configs: the names of CONFIGS, in order.
  net/<cfg>/{pred, grad, target, w_first}: AWAREDetectorNet(**CONFIGS[cfg]) on make_golden_variants' seeded band-limited
      magnitudes [2, 513, 63] (31 pooled rows), one clip per call; pred [2, L, 1] and the band magnitude gradient of each
      clip's push_extremes loss against a seeded bipolar `target` [2, L, 1], every GRAD_STEP-th frame ([2, 225, 8]); w_first
      [blocks, W_FIRST] the first values of every block's conv weight [cout, cin, k] in memory order (the seeded draws).
  traj/<name>/{bits, losses, out_sample, out_step, out_len, raw_marked, det_bits}: the reference's own 400-step embed of
      make_golden's seed clip (TRAJ[name][0] samples) with seeded 20-bit payloads and an edited model card (detection_net_cfg
      with TRAJ[name][1], built as the reference's load() builds it); the waveform every OUT_STEP-th sample.  The tool asserts
      that the reference reads its own payload back without an error before it writes.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_taps.py
"""
import os
import sys
import warnings

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _setup_import_path, make_clip  # noqa: E402
from make_golden_variants import GRAD_STEP, MAG_SEED, MAG_SHAPE, OUT_STEP, magnitudes  # noqa: E402

# detection_net_cfg edits (AWAREDetectorNet keyword arguments); the rest is the card's
CONFIGS = {
    "k3": dict(kernel_size=3),
    "k3_same": dict(kernel_size=3, padding=1),
    "k2": dict(kernel_size=2),
    "k5_p1": dict(kernel_size=5, padding=1, num_blocks=2, n_filters=[256, 256]),
    "k3_s2": dict(kernel_size=3, stride=2, padding=1, num_blocks=1, n_filters=[512]),            # 31 -> 16 -> 8
    "k4_s3": dict(kernel_size=4, stride=3, padding=1, num_blocks=1, n_filters=[250]),            # 31 -> 10 -> 3
    "k3_odd": dict(kernel_size=3, n_mels=13, num_blocks=2, n_filters=[30, 61], output_length=7),
    "k3_gelu_batch_sigmoid": dict(kernel_size=3, padding=1, n_mels=64, num_blocks=2, n_filters=[100, 202], activation="gelu",
                                  norm_layer="batch", final_activation="sigmoid"),
    "k7_p3": dict(kernel_size=7, padding=3, num_blocks=1, n_filters=[128]),
}
# name -> (clip samples, detection_net_cfg edit)
TRAJ = {
    "k3": (16000, dict(kernel_size=3)),
    "k3_s2": (48000, dict(kernel_size=3, stride=2, padding=1, num_blocks=2, n_filters=[256, 256])),    # 93 -> 47 -> 24 -> 12
}
BITS_SEED = 910
W_FIRST = 8


def targets(i, L):
    rng = np.random.default_rng(MAG_SEED + 200 + i)
    return np.where(rng.integers(0, 2, (MAG_SHAPE[0], L, 1)) > 0, 1.0, -1.0).astype(np.float32)


def traj_bits(i):
    return np.random.default_rng(BITS_SEED + i).integers(0, 2, 20).astype(np.int32)


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
    warnings.simplefilter("ignore")
    d = {"mag_seed": MAG_SEED, "mag_shape": np.asarray(MAG_SHAPE), "grad_step": GRAD_STEP, "configs": np.asarray(list(CONFIGS))}
    mag0 = torch.from_numpy(magnitudes())
    for i, (name, kw) in enumerate(CONFIGS.items()):
        net = AWAREDetectorNet(**kw).eval()
        for p in net.parameters():
            p.requires_grad = False
        L = kw.get("output_length", 20)
        target = torch.from_numpy(targets(i, L))
        preds, grads = [], []
        for b in range(MAG_SHAPE[0]):
            mag = mag0[b:b + 1].clone().requires_grad_(True)
            pred = net(mag)
            PushToExtremesLoss()(pred, target[b:b + 1]).backward()
            preds.append(pred.detach().numpy()[0])
            grads.append(mag.grad.numpy()[0, 32:257, ::GRAD_STEP].copy())
        key = f"net/{name}"
        d[key + "/pred"] = np.stack(preds)
        d[key + "/grad"] = np.stack(grads)
        d[key + "/target"] = target.numpy()
        d[key + "/w_first"] = np.stack([blk.conv.weight.detach().numpy().reshape(-1)[:W_FIRST] for blk in net.conv_blocks])
        print(key, d[key + "/pred"][0, :4, 0], flush=True)

    card = yaml.safe_load(open(os.path.join(REF, "src", "AWARE", "cards", "config.yaml")))
    for i, (name, (n, kw)) in enumerate(TRAJ.items()):
        audio, _ = make_clip(1, n)
        bits = traj_bits(i)
        cfg = dict(card)
        cfg["detection_net_cfg"] = dict(card["detection_net_cfg"], **kw)
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
        key = f"traj/{name}"
        d[key + "/bits"] = bits
        d[key + "/n"] = n
        d[key + "/losses"] = np.asarray(losses, np.float64)
        d[key + "/out_len"] = wm_audio.shape[0]
        d[key + "/out_step"] = OUT_STEP
        d[key + "/out_sample"] = wm_audio[::OUT_STEP].astype(np.float32)
        d[key + "/raw_marked"] = detector.detect(wm_audio, 16000).astype(np.float32)
        d[key + "/det_bits"] = np.asarray(detect_watermark(wm_audio, 16000, detector))
        print(key, "loss0", losses[0], "best", min(losses), "bits", bits.tolist(), "det", d[key + "/det_bits"].tolist(),
              flush=True)
        assert np.array_equal(np.asarray(d[key + "/det_bits"]).reshape(-1), bits), f"{name}: the reference's BER is not 0"
    np.savez_compressed(os.path.join(OUT, "detector_taps.npz"), **d)
    print("written", os.path.abspath(os.path.join(OUT, "detector_taps.npz")))


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("reference tree not present: this script only runs in the development container")
    main()
