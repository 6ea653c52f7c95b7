"""Times detectors with temporal convolutions (detection_net_cfg kernel_size / stride / padding, key temporal_convs) beside
the model card's network.

Per detector, 256 clips x 3 s at 16 kHz:
  - one embed iteration: aware_embed_iterate of a recorded graph (16 loop bodies per replay), per-iteration time;
  - aware_detect on the same clips;
  - the workspace the embed session needs;
  - the bytes one embed iteration moves through the unfold and fold kernels (what they read and write, by the kernels'
    definition: unfold reads its block's valid input rows once and writes every row of U up to the clips' 32-row boundaries;
    fold reads the valid rows of dU and writes every row of dX).
HIP-event timing, warm-up, median over repetitions.  Prints one JSON line per detector.
    python tools/detector_taps_bench.py [--reps 10] [--clips 256] [--seconds 3] [--only KEY] [--out FILE]
KEY: card, k3, k3_same, k3_s2.
`--trace KEY` times nothing: it runs 20 embed iterations of that detector without a graph, for a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/detector_taps_bench.py --trace k3), whose conv_unfold_kernel and
conv_fold_kernel rows divide into the bytes above.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NETS = {"card": {}, "k3": dict(kernel_size=3), "k3_same": dict(kernel_size=3, padding=1),
        "k3_s2": dict(kernel_size=3, stride=2, padding=1, num_blocks=2, n_filters=[256, 256])}
GRAPH_ITERS = 16
TRACE_ITERS = 20


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


def tap_bytes(net, rt, batch):
    """(unfold bytes, fold bytes) of one forward + backward of `net` on `batch`."""
    if not net.has_taps:
        return 0, 0
    stored = rt.stored_channels(net.channels)
    k = net.kernel_size
    padded = batch.total_pooled
    unfold = fold = 0
    for blk, cs in enumerate(stored[:-1]):
        rows_in = sum(net.block_rows(t // 2)[blk] for t in batch.frames)
        rows_out = sum(net.block_rows(t // 2)[blk + 1] for t in batch.frames)
        unfold += 4 * cs * (rows_in + k * padded)
        fold += 4 * cs * (k * rows_out + padded)
    return unfold, fold


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--only", default=None, choices=list(NETS))
    ap.add_argument("--trace", default=None, choices=list(NETS))
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
    if args.trace:
        net = AWAREDetectorNet(temporal_convs=True, **NETS[args.trace])
        sess = rt.EmbedSession(plan, net.device_weights(plan), batch, num_iterations=TRACE_ITERS, use_graph=False)
        sess.begin(audio, wm)
        sess.iterate(TRACE_ITERS)
        torch.cuda.synchronize()
        u, f = tap_bytes(net, rt, batch)
        print(json.dumps({"detector": args.trace, "iterations": TRACE_ITERS, "unfold_bytes_per_iteration": u,
                          "fold_bytes_per_iteration": f, "blocks": net.num_blocks + 1}), flush=True)
        return
    iters = (2 + args.reps) * GRAPH_ITERS
    lines = []
    for key, kw in NETS.items():
        if args.only and key != args.only:
            continue
        net = AWAREDetectorNet(temporal_convs=True, **kw)
        det = net.device_weights(plan)
        sess = rt.EmbedSession(plan, det, batch, num_iterations=iters, use_graph=True)
        sess.begin(audio, wm)
        it_ms = median_ms(lambda: sess.iterate(GRAPH_ITERS), args.reps) / GRAPH_ITERS
        det_ms = median_ms(lambda: rt.detect(plan, det, batch, audio), args.reps)
        u, f = tap_bytes(net, rt, batch)
        line = {"detector": key, "conv": [net.kernel_size, net.stride, net.padding], "channels": net.channels,
                "rows": net.block_rows(batch.frames[0] // 2), "clips": args.clips, "seconds": args.seconds,
                "embed_iteration_ms": round(it_ms, 3), "detect_ms": round(det_ms, 3),
                "embed_workspace_mb": round(plan.lib.aware_embed_workspace_bytes(batch.h, det.h) / 1e6, 1),
                "unfold_mb_per_iteration": round(u / 1e6, 1), "fold_mb_per_iteration": round(f / 1e6, 1),
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
