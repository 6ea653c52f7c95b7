"""Times detectors with another initial pool (detection_net_cfg initial_pool_size / initial_pool_stride, key initial_pools)
beside the model card's network.

Per detector, 256 clips x 3 s at 16 kHz:
  - the rows per block, one embed iteration (aware_embed_iterate of a recorded graph, 16 loop bodies per replay, per-iteration
    time), aware_detect on the same clips, and the workspace the embed session needs;
  - the bytes one embed iteration moves through the three kernels of mel_pool_kernels.hip, by the kernels' definition: the
    forward reads xm once and writes every row of x0 up to the clips' 32-row boundaries; the backward partial kernel reads xm
    and the valid rows of dx0; the backward apply kernel reads both again and writes xm.
HIP-event timing, warm-up, median over repetitions.  Prints one JSON line per detector.
    python tools/detector_pool_bench.py [--reps 10] [--clips 256] [--seconds 3] [--only KEY] [--out FILE]
KEY: card, key22 (the key at (2, 2): the card's route), p44, p32, p88, and staged22 -- the card's blocks on the staged route
after the (2, 2) pool (a sigmoid read-out is all that keeps it off the fused kernels): the like-for-like baseline for what
fewer rows buy.
`--trace KEY` times nothing: it runs 20 embed iterations of that detector without a graph, for a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/detector_pool_bench.py --trace p44), whose mel_pool_* rows divide into the
bytes above.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pool(size, stride):
    return dict(initial_pool_size=size, initial_pool_stride=stride)


NETS = {"card": None, "key22": pool(2, 2), "p44": pool(4, 4), "p32": pool(3, 2), "p88": pool(8, 8),
        "staged22": dict(pool(2, 2), final_activation="sigmoid")}
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


def make_net(key):
    from aware_amd.detection import AWAREDetectorNet
    return AWAREDetectorNet() if NETS[key] is None else AWAREDetectorNet(initial_pools=True, **NETS[key])


def pool_bytes(net, rt, batch):
    """(forward, backward partial, backward apply) bytes of the mel_pool kernels in one iteration of `net` on `batch`."""
    if not net.has_pool:
        return 0, 0, 0
    mp = rt.stored_channels(net.channels)[0]
    xm = 4 * mp * batch.total_frames
    rows = sum(net.pooled_rows(t) for t in batch.frames)
    return xm + 4 * mp * batch.total_pooled, xm + 4 * mp * rows, 2 * xm + 4 * mp * rows


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
        net = make_net(args.trace)
        sess = rt.EmbedSession(plan, net.device_weights(plan), batch, num_iterations=TRACE_ITERS, use_graph=False)
        sess.begin(audio, wm)
        sess.iterate(TRACE_ITERS)
        torch.cuda.synchronize()
        f, bp, ba = pool_bytes(net, rt, batch)
        print(json.dumps({"detector": args.trace, "iterations": TRACE_ITERS, "pool_fwd_bytes_per_iteration": f,
                          "pool_bwd_partial_bytes_per_iteration": bp, "pool_bwd_apply_bytes_per_iteration": ba,
                          "blocks": net.num_blocks + 1}), flush=True)
        return
    iters = (2 + args.reps) * GRAPH_ITERS
    lines = []
    for key in NETS:
        if args.only and key != args.only:
            continue
        net = make_net(key)
        det = net.device_weights(plan)
        sess = rt.EmbedSession(plan, det, batch, num_iterations=iters, use_graph=True)
        sess.begin(audio, wm)
        it_ms = median_ms(lambda: sess.iterate(GRAPH_ITERS), args.reps) / GRAPH_ITERS
        det_ms = median_ms(lambda: rt.detect(plan, det, batch, audio), args.reps)
        f, bp, ba = pool_bytes(net, rt, batch)
        line = {"detector": key, "pool": list(net.pool), "is_card": det.is_card, "channels": net.channels,
                "rows": net.block_rows(net.pooled_rows(batch.frames[0])), "clips": args.clips, "seconds": args.seconds,
                "embed_iteration_ms": round(it_ms, 3), "detect_ms": round(det_ms, 3),
                "embed_workspace_mb": round(plan.lib.aware_embed_workspace_bytes(batch.h, det.h) / 1e6, 1),
                "pool_fwd_mb_per_iteration": round(f / 1e6, 1), "pool_bwd_partial_mb_per_iteration": round(bp / 1e6, 1),
                "pool_bwd_apply_mb_per_iteration": round(ba / 1e6, 1), "loss_finite": bool(torch.isfinite(sess.loss).all())}
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
