"""Times the speed search in detection.

On `--clips` clips of `--seconds` at 16 kHz and the grid `--max-percent` / `--step-percent`:
  - aware_speed_views: all views in one launch (LDS staging);
  - aware_speed_change on the same views as pseudo-clips (every clip once per view, overlapping x_off): the gather form;
  - AWAREDetector.detect_batch plain, with the speed search, and with sync_search = 8 (wall time to a synchronise).
The two kernels are alternated in rounds of `--reps` launches between HIP events, after a warm-up and a bit-for-bit comparison of
their outputs.  Prints one JSON line.
    python tools/speed_search_bench.py [--clips 64] [--seconds 1] [--max-percent 12] [--step-percent 0.5] [--reps 200] [--rounds 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return {"median": round(float(np.median(v)), 2), "min": round(float(min(v)), 2), "max": round(float(max(v)), 2)}


def wall_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--max-percent", type=float, default=12.0)
    ap.add_argument("--step-percent", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    from aware_amd import _lib, runtime as rt
    from aware_amd.detection import sync as S
    from aware_amd.embedding import loop_attacks as LA
    from aware_amd.utils.models import load
    rt.require_gpu()
    lib = _lib.load_library()
    search = {"max_percent": args.max_percent, "step_percent": args.step_percent}
    ms = S.speed_offsets(search)
    B, N, V = args.clips, int(16000 * args.seconds), len(ms)
    rng = np.random.default_rng(0)
    clips = [(0.1 * rng.standard_normal(N)).astype(np.float32) for _ in range(B)]
    x = rt.Ragged.from_list(clips)
    dev = x.data.device
    vlen = [LA.speed_length(N, m) for _ in range(B) for m in ms]
    voff = np.concatenate([[0], np.cumsum([(n + 3) // 4 * 4 for n in vlen])]).astype(np.int64)
    ints = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    md, od, z_len = ints(ms), ints(voff[:-1]), ints(vlen)
    p_off, p_len, p_m = ints([x.offsets[b] for b in range(B) for _ in ms]), ints([N] * (B * V)), ints(ms * B)
    outs = {k: torch.zeros(int(voff[-1]), dtype=torch.float32, device=dev) for k in ("speed_views", "speed_change")}
    P, st = rt._ptr, rt._stream

    def run(kind):
        if kind == "speed_views":
            rc = lib.aware_speed_views(P(x.data), P(x.d_off), P(x.d_len), B, P(md), V, P(outs[kind]), P(od), max(vlen), st())
        else:
            rc = lib.aware_speed_change(P(x.data), P(p_off), P(p_len), P(outs[kind]), P(od), P(z_len), B * V, max(vlen), P(p_m), 0, st())
        _lib.check(rc, kind)

    for k in outs:
        for _ in range(20):
            run(k)
    torch.cuda.synchronize()
    if not torch.equal(outs["speed_views"], outs["speed_change"]):
        raise RuntimeError("aware_speed_views and aware_speed_change differ")
    us = {k: [] for k in outs}
    for _ in range(args.rounds):
        for k in outs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                run(k)
            b.record()
            b.synchronize()
            us[k].append(a.elapsed_time(b) / args.reps * 1e3)
    _, det = load()
    line = {"clips": B, "samples": N, "views": V, "view_samples": int(sum(vlen)),
            "us_per_launch": {k: spread(v) for k, v in us.items()},
            # one write of the views and one read of the clips
            "speed_views_gb_per_s": round(4.0 * (sum(vlen) + B * N) / (float(np.median(us["speed_views"])) * 1e-6) / 1e9, 1),
            "detect_batch_ms": {"plain": wall_ms(lambda: det.detect_batch(clips, 16000)),
                                "speed_search": wall_ms(lambda: det.detect_batch(clips, 16000, speed_search=search)),
                                "sync_search_8": wall_ms(lambda: det.detect_batch(clips, 16000, sync_search=8))}}
    line["speed_views_share_of_searching_call"] = round(
        float(np.median(us["speed_views"])) * 1e-3 / line["detect_batch_ms"]["speed_search"], 4)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
