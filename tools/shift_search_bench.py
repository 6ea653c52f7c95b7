"""Times the shift search in detection.

On `--clips` clips of `--seconds` at 16 kHz and the grid `--max-hz` / `--step-hz`:
  - aware_shift_views: all views in one launch, the Hilbert transform once per clip;
  - aware_frequency_shift once per view into the same rows (the clips laid out at the rows' stride, so that one launch
    serves view j of every clip): what the library could do before the views kernel;
  - AWAREDetector.detect_batch plain and detect_batch_shift with the search (wall time to a synchronise).
The two forms are alternated in `--rounds` windows of `--reps` repetitions between HIP events, after a warm-up and a bit-for-bit
comparison of their outputs.  Prints one JSON line.
    python tools/shift_search_bench.py [--clips 256] [--seconds 3] [--max-hz 150] [--step-hz 10] [--reps 20] [--rounds 3]
"""
import argparse
import ctypes as C
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


def wall_ms(fn, reps=3):
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
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--max-hz", type=float, default=150.0)
    ap.add_argument("--step-hz", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-detect", action="store_true", help="time the two view forms only")
    args = ap.parse_args()
    from aware_amd import _lib, runtime as rt
    from aware_amd.detection import sync as S
    from aware_amd.utils.models import load
    rt.require_gpu()
    lib = _lib.load_library()
    search = {"max_hz": args.max_hz, "step_hz": args.step_hz}
    ds = S.shift_offsets(search, 16000)
    B, N, V = args.clips, int(16000 * args.seconds) // 4 * 4, len(ds)         # rows of whole float4s: both forms write the same floats
    rng = np.random.default_rng(0)
    clips = [(0.1 * rng.standard_normal(N)).astype(np.float32) for _ in range(B)]
    x = rt.Ragged.from_list(clips)
    dev = x.data.device
    ints = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    dd, od = ints(ds), ints([r * N for r in range(B * V)])
    # the per-view form: aware_frequency_shift reads and writes clip b at the same offset, so the clips lie V rows apart
    wide = torch.zeros(B * V * N, dtype=torch.float32, device=dev)
    wide.view(B, V * N)[:, :N] = torch.from_numpy(np.stack(clips)).to(dev)
    w_off, w_len, zero = ints([b * V * N for b in range(B)]), ints([N] * B), ints([0] * B)
    per_d = [ints([d] * B) for d in ds]
    outs = {k: torch.zeros(B * V * N, dtype=torch.float32, device=dev) for k in ("shift_views", "frequency_shift_per_view")}
    P, st = rt._ptr, rt._stream

    def run(kind):
        if kind == "shift_views":
            _lib.check(lib.aware_shift_views(P(x.data), P(x.d_off), P(x.d_len), B, P(dd), V, P(outs[kind]), P(od), N, st()), kind)
        else:
            for j in range(V):
                _lib.check(lib.aware_frequency_shift(P(wide), P(w_off), P(w_len), B, N, P(per_d[j]), P(zero), 0,
                                                     C.c_void_p(outs[kind].data_ptr() + 4 * j * N), st()), kind)

    for k in outs:
        for _ in range(3):
            run(k)
    torch.cuda.synchronize()
    if not torch.equal(outs["shift_views"], outs["frequency_shift_per_view"]):
        raise RuntimeError("aware_shift_views and aware_frequency_shift differ")
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
    line = {"clips": B, "samples": N, "views": V, "view_samples": B * V * N,
            "us_per_all_views": {k: spread(v) for k, v in us.items()},
            # the stores alone: B V N floats
            "store_gb_per_s": {k: round(4.0 * B * V * N / (float(np.median(v)) * 1e-6) / 1e9, 1) for k, v in us.items()}}
    if not args.no_detect:
        del outs, wide
        _, det = load()
        line["detect_batch_ms"] = {"plain": wall_ms(lambda: det.detect_batch(clips, 16000)),
                                   "shift_search": wall_ms(lambda: det.detect_batch_shift(clips, 16000, shift_search=search))}
        line["shift_views_share_of_searching_call"] = round(
            float(np.median(us["shift_views"])) * 1e-3 / line["detect_batch_ms"]["shift_search"], 4)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
