"""Times the scan of long recordings.

On `--files` files of `--seconds` of unmarked Gaussian audio at 16 kHz and the scan's defaults (windows of 1 s every 4096
samples at 8 sync offsets):
  - AWAREDetector.scan as a whole (wall time to a synchronise, upload and host work included), and the audio it reads per second;
  - the aware_detect calls of that scan between HIP events (the calls alone: the time from the first launch of a call to its
    last, summed over the calls of one scan);
  - aware_scan_select and aware_scan_segments on that scan's own values, `--reps` launches between HIP events, in `--rounds`.
Prints one JSON line.
    python tools/scan_bench.py [--files 8] [--seconds 60] [--reps 200] [--rounds 7]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    from aware_amd import _lib, runtime as rt
    from aware_amd.utils.models import load
    rt.require_gpu()
    lib = _lib.load_library()
    _, det = load()
    rng = np.random.default_rng(0)
    N = int(16000 * args.seconds)
    files = [(0.1 * rng.standard_normal(N)).astype(np.float32) for _ in range(args.files)]

    # the scan's own intermediate values, and its aware_detect calls between events
    kept, detect_ms = {}, []
    real = {"detect": rt.detect, "scan_select": rt.scan_select, "scan_segments": rt.scan_segments}

    def detect(*a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = real["detect"](*a)
        e1.record()
        detect_ms[-1].append((e0, e1))
        return out

    def scan_select(values, win_off, n, centre):
        kept.update(values=values, win_off=win_off, n=n, centre=centre)
        kept["select"] = real["scan_select"](values, win_off, n, centre)
        return kept["select"]

    def scan_segments(*a, **kw):
        kept["segments_args"] = a
        return real["scan_segments"](*a, **kw)

    rt.detect, rt.scan_select, rt.scan_segments = detect, scan_select, scan_segments
    try:
        wall = []
        for i in range(1 + args.rounds):                       # the first scan warms up
            detect_ms.append([])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            spans, profiles = det.scan(files, 16000, return_profile=True)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
    finally:
        rt.detect, rt.scan_select, rt.scan_segments = real["detect"], real["scan_select"], real["scan_segments"]
    wall, detect_ms = wall[1:], [sum(a.elapsed_time(b) for a, b in calls) for calls in detect_ms[1:]]
    calls = len(kept["values"]) // det.scan_rows_per_call + bool(len(kept["values"]) % det.scan_rows_per_call)

    values, win_off, n, centre = kept["values"], kept["win_off"], kept["n"], kept["centre"]
    out, view, conf, bits = kept["select"]
    _, _, _, _, _, _, min_conf, max_flip, S = kept["segments_args"]
    arr, B, W = rt._scan_offsets(win_off, "scan_bench")
    L = int(values.shape[1])
    dev = values.device
    off_dev = torch.tensor(list(arr), dtype=torch.int32, device=dev)
    seg_i = [torch.empty((B, S), dtype=torch.int32, device=dev) for _ in range(4)]
    n_seg = torch.empty(B, dtype=torch.int32, device=dev)
    seg_c, seg_v = torch.empty((B, S), device=dev), torch.empty((B, S, L), device=dev)
    P, st = rt._ptr, rt._stream

    def run(kind):
        if kind == "scan_select":
            rc = lib.aware_scan_select(P(values), arr, B, n, L, centre, P(conf), P(view), P(out), P(bits), st())
        else:
            rc = lib.aware_scan_segments(P(conf), P(view), P(out), P(bits), arr, P(off_dev), B, L, centre, float(min_conf),
                                         int(max_flip), int(S), P(n_seg), P(seg_i[0]), P(seg_i[1]), P(seg_i[2]), P(seg_i[3]),
                                         P(seg_c), P(seg_v), st())
        _lib.check(rc, kind)

    us = {"scan_select": [], "scan_segments": []}
    for k in us:
        for _ in range(20):
            run(k)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k in us:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                run(k)
            b.record()
            b.synchronize()
            us[k].append(a.elapsed_time(b) / args.reps * 1e3)
    line = {"files": args.files, "seconds": args.seconds, "windows": W, "rows": int(values.shape[0]), "n_bits": L,
            "aware_detect_calls": calls, "spans": sum(len(s) for s in spans),
            "largest_win_conf": round(float(max(p["win_conf"].max() for p in profiles)), 4),
            "scan_ms": spread(wall),
            "audio_seconds_per_second": round(args.files * args.seconds / (float(np.median(wall)) * 1e-3), 1),
            "aware_detect_ms_per_scan": spread(detect_ms),
            "us_per_launch": {k: spread(v) for k, v in us.items()}}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
