#!/usr/bin/env python3
"""Generate tests/golden/detector_pool.npz by running the reference's detector with other initial pools on the CPU.

TEST INFRASTRUCTURE, like tools/make_golden_taps.py (same import recipe and stand-ins, imported from tools/make_golden.py):
it runs only where the reference tree exists and writes data only.  Contents:

  configs: the names of CONFIGS, in order; pool/<cfg>: (initial_pool_size, initial_pool_stride).
  net/<cfg>/{pred, grad, target, w_first}: AWAREDetectorNet(**CONFIGS[cfg]) on make_golden_variants' seeded band-limited
      magnitudes [2, 513, 63], one clip per call; pred [2, L, 1] and the band magnitude gradient of each clip's push_extremes
      loss against a seeded bipolar `target` [2, L, 1], every GRAD_STEP-th frame ([2, 225, 8]); w_first [blocks, W_FIRST] the
      first values of every block's conv weight in memory order (the seeded draws: the pool has no weights, so they are those
      of the same net after the (2, 2) pool).
  traj/<name>/{bits, losses, out_sample, out_step, out_len, raw_marked, det_bits, ber}: the reference's own 400-step embed of
      make_golden's seed clip (TRAJ[name][0] samples) with seeded 20-bit payloads and an edited model card (detection_net_cfg
      with TRAJ[name][1], built as the reference's load() builds it); the waveform every OUT_STEP-th sample.  `p44` on 1 s is
      always written; of the overlapping pools on 3 s (OVERLAP, in order) the first at which the reference reads its own
      payload back without an error.  traj_tried/<name>: the bit errors the reference read at every trajectory it ran.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_pool.py
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


def pool(size, stride):
    return dict(initial_pool_size=size, initial_pool_stride=stride)


# detection_net_cfg edits (AWAREDetectorNet keyword arguments); the rest is the card's.  63 frames -> rows in the comments
CONFIGS = {
    "p44": pool(4, 4),                                                                            # 15
    "p32": pool(3, 2),                                                                            # 31, overlapping
    "p23": pool(2, 3),                                                                            # 21, gaps
    "p82": pool(8, 2),                                                                            # 28, four windows per frame
    "p88": pool(8, 8),                                                                            # 7
    "p33_small": dict(pool(3, 3), n_mels=80, num_blocks=2, n_filters=[72, 64], activation="gelu", norm_layer="batch",
                      final_activation="sigmoid"),                                               # 21
    "p44_k3": dict(pool(4, 4), kernel_size=3, stride=1, padding=1),                               # 15 in every block
}
# name -> (clip samples, detection_net_cfg edit)
TRAJ = {"p44": (16000, pool(4, 4))}
OVERLAP = {"p32": (48000, pool(3, 2)), "p82": (48000, pool(8, 2))}
BITS_SEED = 1010
W_FIRST = 8


def targets(i, L):
    rng = np.random.default_rng(MAG_SEED + 300 + i)
    return np.where(rng.integers(0, 2, (MAG_SHAPE[0], L, 1)) > 0, 1.0, -1.0).astype(np.float32)


def traj_bits(name):
    return np.random.default_rng(BITS_SEED + list(CONFIGS).index(name)).integers(0, 2, 20).astype(np.int32)


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
        d[f"pool/{name}"] = np.asarray([kw["initial_pool_size"], kw["initial_pool_stride"]])
        d[key + "/pred"] = np.stack(preds)
        d[key + "/grad"] = np.stack(grads)
        d[key + "/target"] = target.numpy()
        d[key + "/w_first"] = np.stack([blk.conv.weight.detach().numpy().reshape(-1)[:W_FIRST] for blk in net.conv_blocks])
        print(key, d[key + "/pred"][0, :4, 0], flush=True)

    card = yaml.safe_load(open(os.path.join(REF, "src", "AWARE", "cards", "config.yaml")))

    def trajectory(name, n, kw):
        audio, _ = make_clip(1, n)
        bits = traj_bits(name)
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
        t = {"bits": bits, "n": n, "losses": np.asarray(losses, np.float64), "out_len": wm_audio.shape[0], "out_step": OUT_STEP,
             "out_sample": wm_audio[::OUT_STEP].astype(np.float32),
             "raw_marked": detector.detect(wm_audio, 16000).astype(np.float32),
             "det_bits": np.asarray(detect_watermark(wm_audio, 16000, detector))}
        t["ber"] = int(np.sum(t["det_bits"].reshape(-1) != bits))
        print(f"traj/{name}", "loss0", losses[0], "best", min(losses), "bits", bits.tolist(), "det", t["det_bits"].tolist(),
              "errors", t["ber"], flush=True)
        return t

    def keep(name, t):
        for k, v in t.items():
            d[f"traj/{name}/{k}"] = v

    for name, (n, kw) in TRAJ.items():
        t = trajectory(name, n, kw)
        d[f"traj_tried/{name}"] = t["ber"]
        keep(name, t)
    for name, (n, kw) in OVERLAP.items():
        t = trajectory(name, n, kw)
        d[f"traj_tried/{name}"] = t["ber"]
        if t["ber"] == 0:
            keep(name, t)
            break
    else:
        sys.exit("no overlapping pool at which the reference's BER is 0")
    d["traj"] = np.asarray(sorted({k.split("/")[1] for k in d if k.startswith("traj/")}))
    np.savez_compressed(os.path.join(OUT, "detector_pool.npz"), **d)
    print("written", os.path.abspath(os.path.join(OUT, "detector_pool.npz")))


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("reference tree not present: this script only runs in the development container")
    main()
