"""Times the embed loop and detection at payload lengths of 20 .. 512 bits (watermark_length / output_length).

Per length, config 3's batch (256 clips x 3 s at 16 kHz) on the model card's network with an L-bit read-out:
  - one embed iteration: aware_embed_iterate of a recorded graph (16 loop bodies per replay), per-iteration time, and the
    waveform-seconds per second of a 400-iteration embed at that rate;
  - aware_detect on the same clips.
HIP-event timing, warm-up, median over repetitions.  Prints one JSON line per length.
    python tools/payload_bench.py [--reps 10] [--clips 256] [--seconds 3] [--only L] [--out FILE]
For the wide read-out kernel's time (readout_wide_kernel), run it under rocprofv3:
    rocprofv3 --kernel-trace --stats -d DIR -o payload -- python tools/payload_bench.py --reps 2 --only 64
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTHS = [20, 33, 64, 128, 512]
GRAPH_ITERS = 16
EMBED_ITERS = 400


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
    ap.add_argument("--only", type=int, default=None, help="one payload length in bits")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from aware_amd import runtime as rt
    from aware_amd.detection import AWAREDetectorNet
    from aware_amd.utils.audio import default_plan
    rt.require_gpu()
    n = int(16000 * args.seconds)
    rng = np.random.default_rng(0)
    clips = [(0.1 * rng.standard_normal(n)).astype(np.float32) for _ in range(args.clips)]
    batch = rt.Batch([n] * args.clips)
    audio = batch.pack(clips)
    plan = default_plan()
    iters = (2 + args.reps) * GRAPH_ITERS
    lines = []
    for L in (LENGTHS if args.only is None else [args.only]):
        det = AWAREDetectorNet(output_length=L).device_weights(plan)
        wm = torch.from_numpy(np.where(rng.integers(0, 2, (args.clips, L)) > 0, 1.0, -1.0).astype(np.float32)).cuda()
        sess = rt.EmbedSession(plan, det, batch, num_iterations=iters, use_graph=True)
        sess.begin(audio, wm)
        it_ms = median_ms(lambda: sess.iterate(GRAPH_ITERS), args.reps) / GRAPH_ITERS
        det_ms = median_ms(lambda: rt.detect(plan, det, batch, audio), args.reps)
        line = {"bits": L, "last_block_channels": 2 * L, "clips": args.clips, "seconds": args.seconds,
                "embed_iteration_ms": round(it_ms, 3), "detect_ms": round(det_ms, 3),
                "embed_wf_s_per_s": round(args.clips * args.seconds / (EMBED_ITERS * it_ms / 1e3), 1),
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
