"""Times detectors of other sizes (detection_net_cfg n_mels, num_blocks, n_filters) against the model card's network.

Per detector, 256 clips x 3 s at 16 kHz:
  - one embed iteration: aware_embed_iterate of a recorded graph (16 loop bodies per replay), per-iteration time;
  - aware_detect on the same clips;
  - the workspace the embed session needs.
HIP-event timing, warm-up, median over repetitions.  Prints one JSON line per detector.
    python tools/detector_sizes_bench.py [--reps 10] [--clips 256] [--seconds 3] [--only KEY] [--out FILE]
KEY: card, m40, m64, m200, f_odd, deep10.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"card": {}, "m40": dict(n_mels=40), "m64": dict(n_mels=64), "m200": dict(n_mels=200),
         "f_odd": dict(n_filters=[250, 500, 750]), "deep10": dict(num_blocks=10, n_filters=[256] * 10)}
GRAPH_ITERS = 16


def median_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--only", default=None, choices=list(SIZES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from aware_amd import runtime as rt
    from aware_amd.detection import AWAREDetectorNet
    from aware_amd.utils.audio import default_plan
    rt.require_gpu()
    plan = default_plan()
    n = int(16000 * args.seconds)
    rng = np.random.default_rng(0)
    clips = [(0.1 * rng.standard_normal(n)).astype(np.float32) for _ in range(args.clips)]
    batch = rt.Batch([n] * args.clips)
    audio = batch.pack(clips)
    wm = torch.from_numpy(np.where(rng.integers(0, 2, (args.clips, 20)) > 0, 1.0, -1.0).astype(np.float32)).cuda()
    iters = (2 + args.reps) * GRAPH_ITERS
    lines = []
    for key, kw in SIZES.items():
        if args.only and key != args.only:
            continue
        net = AWAREDetectorNet(**kw)
        det = net.device_weights(plan)
        sess = rt.EmbedSession(plan, det, batch, num_iterations=iters, use_graph=True)
        sess.begin(audio, wm)
        it_ms = median_ms(lambda: sess.iterate(GRAPH_ITERS), args.reps) / GRAPH_ITERS
        det_ms = median_ms(lambda: rt.detect(plan, det, batch, audio), args.reps)
        line = {"detector": key, "channels": net.channels, "stored": rt.stored_channels(net.channels), "clips": args.clips,
                "seconds": args.seconds, "embed_iteration_ms": round(it_ms, 3), "detect_ms": round(det_ms, 3),
                "embed_workspace_mb": round(plan.lib.aware_embed_workspace_bytes(batch.h, det.h) / 1e6, 1),
                "loss_finite": bool(torch.isfinite(sess.loss).all())}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del sess
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
