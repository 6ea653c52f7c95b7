"""STOI timing: on 256 x 3 s clips and on the ragged 1..10 s batch of BASELINE config 5,
  (a) rt.stoi on the device with HIP events, median of 10 after a warm-up of every shape, with the resampling to 10 kHz and
      without it (the same signals already at 10 kHz);
  (b) the only route to the same numbers without it: copy both batches to the host and loop metrics.audio.stoi (host clock;
      --host-clips N bounds the loop and scales the total, 0 skips it);
  (c) one embed step (400 iterations) of the same batch, for scale.
`--only-stoi` runs (a) alone, a few calls, for a per-kernel trace (rocprofv3 --kernel-trace --stats -- python tools/stoi_bench.py --only-stoi)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aware_amd import runtime as rt
from aware_amd.metrics import audio as M


def event_ms(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def make_batch(lengths, seed):
    """white-noise clips (the benchmark's workload) and a processed copy 20 dB below them"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = 0.1 * torch.randn(sum(lengths), generator=g, device="cuda")
    y = x + 0.01 * torch.randn(sum(lengths), generator=g, device="cuda")
    return rt.Ragged(y, lengths), rt.Ragged(x, lengths)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-clips", type=int, default=16)
    ap.add_argument("--only-stoi", action="store_true")
    ap.add_argument("--no-embed", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(20250905)
    shapes = {"256 x 3 s": [48000] * 256, "config 5 (256 clips of 1..10 s)": [int(s) * 16000 for s in rng.integers(1, 11, 256)]}
    for name, lengths in shapes.items():
        out, tgt = make_batch(lengths, 1)
        secs = sum(lengths) / 16000.0
        with_rs = event_ms(lambda: rt.stoi(out, tgt, 16000), reps=3 if args.only_stoi else 10)
        l10 = [-(-n * 5 // 8) for n in lengths]
        out10, tgt10 = make_batch(l10, 2)
        without = event_ms(lambda: rt.stoi(out10, tgt10, 10000), reps=3 if args.only_stoi else 10)
        print(f"{name}: {secs:.0f} s of audio")
        print(f"  (a) rt.stoi, resampling included: median {with_rs[0]:.3f} ms (min {with_rs[1]:.3f}, max {with_rs[2]:.3f})")
        print(f"  (a) rt.stoi, already at 10 kHz:   median {without[0]:.3f} ms (min {without[1]:.3f}, max {without[2]:.3f})")
        if args.only_stoi:
            continue
        if args.host_clips > 0:
            t0 = time.perf_counter()
            xs, ys = tgt.to_list(), out.to_list()
            t_copy = time.perf_counter() - t0
            idx = np.linspace(0, len(lengths) - 1, min(args.host_clips, len(lengths))).astype(int)
            M.stoi(xs[0][:16000].astype(np.float64), ys[0][:16000].astype(np.float64), 16000)     # imports, filter design
            t0 = time.perf_counter()
            for i in idx:
                M.stoi(xs[i].astype(np.float64), ys[i].astype(np.float64), 16000)
            t_loop = time.perf_counter() - t0
            scale = sum(lengths) / float(sum(lengths[i] for i in idx))
            print(f"  (b) host: copy {t_copy * 1e3:.1f} ms + loop of metrics.audio.stoi {t_loop * 1e3:.1f} ms for {len(idx)} clips "
                  f"-> {t_loop * scale * 1e3:.0f} ms for the batch (scaled by samples)")
        if not args.no_embed:
            from aware_amd.utils.models import load
            emb, _ = load()
            batch = rt.Batch(lengths)
            sess = emb.start_session(batch, 16000)
            target = torch.randint(0, 2, (len(lengths), 20), device="cuda").float() * 2 - 1

            def embed():
                sess.begin(tgt.data, target)
                sess.iterate(400)
            t = event_ms(embed, reps=3, warm=1)
            print(f"  (c) embed, 400 iterations of the same batch: median {t[0]:.1f} ms")


if __name__ == "__main__":
    main()
