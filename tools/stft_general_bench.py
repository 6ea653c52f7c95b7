"""Times the general-geometry STFT path (csrc/stft_any.hip) against torch.stft / torch.istft on the same GPU.

Per shape (clips x seconds at 16 kHz, n_fft / hop, hann, win_length = n_fft):
  - end to end: STFT -> ISTFT forward + backward through the plug-ins (autograd.Function over the C ABI) against the same
    chain on torch.stft / torch.istft with autograd, float32 on the GPU;
  - per entry point: aware_stft (analysis kernel), aware_istft (frame + overlap-add kernels), aware_stft_bwd, aware_istft_bwd,
    with the share of 8 TB/s on algorithmic bytes (samples in + spectrum out, or the reverse).
HIP-event timing, warm-up, median over repetitions.  Prints one JSON line per shape.
    python tools/stft_general_bench.py [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8e12
SHAPES = [(256, 3.0, 2048, 512), (64, 10.0, 2048, 512), (256, 3.0, 512, 128), (64, 10.0, 512, 128)]


def median_ms(fn, reps, warmup=3):
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from aware_amd import runtime as rt
    from aware_amd.utils.audio import STFT, ISTFT
    rt.require_gpu()
    lines = []
    for B, sec, n_fft, hop in SHAPES:
        L = int(16000 * sec)
        g = torch.Generator(device="cuda").manual_seed(0)
        x = torch.randn(B, L, device="cuda", generator=g)
        T = 1 + L // hop
        F = n_fft // 2 + 1
        w_out = torch.randn(B, hop * (T - 1), device="cuda", generator=g)
        stft_p, istft_p = STFT(n_fft, hop, "hann", n_fft), ISTFT(n_fft, hop, "hann", n_fft)
        win = torch.hann_window(n_fft, device="cuda")

        def mine():
            xd = x.detach().requires_grad_(True)
            y = istft_p(stft_p(xd))
            (y * w_out).sum().backward()

        def theirs():
            xd = x.detach().requires_grad_(True)
            S = torch.stft(xd, n_fft, hop, n_fft, win, center=True, pad_mode="reflect", return_complex=True)
            y = torch.istft(S, n_fft, hop, n_fft, win, center=True)
            (y * w_out).sum().backward()

        t_mine, t_torch = median_ms(mine, args.reps), median_ms(theirs, args.reps)
        # per entry point on the runtime layer
        plan = rt.Plan(n_fft, hop, n_fft, "hann")
        batch = rt.Batch([L] * B, plan=plan)
        flat = x.reshape(-1).contiguous()
        spec = rt.stft(plan, batch, flat)
        gout = w_out.reshape(-1).contiguous()
        t_an = median_ms(lambda: rt.stft(plan, batch, flat), args.reps)
        t_sy = median_ms(lambda: rt.istft(plan, batch, spec), args.reps)
        t_sb = median_ms(lambda: rt.stft_bwd(plan, batch, spec), args.reps)
        t_ib = median_ms(lambda: rt.istft_bwd(plan, batch, gout), args.reps)
        sig_bytes, out_bytes, spec_bytes = B * L * 4, batch.total_out * 4, batch.total_frames * F * 8
        frac = lambda nbytes, ms: nbytes / (ms * 1e-3) / HBM
        rec = {"clips": B, "seconds": sec, "n_fft": n_fft, "hop": hop, "frames": batch.total_frames,
               "fwd_bwd_ms": {"aware": round(t_mine, 3), "torch": round(t_torch, 3), "speedup": round(t_torch / t_mine, 2)},
               "entry_ms": {"stft": round(t_an, 3), "istft": round(t_sy, 3), "stft_bwd": round(t_sb, 3), "istft_bwd": round(t_ib, 3)},
               "frac_8TBs": {"stft": round(frac(sig_bytes + spec_bytes, t_an), 3), "istft": round(frac(spec_bytes + out_bytes, t_sy), 3),
                             "stft_bwd": round(frac(spec_bytes + sig_bytes, t_sb), 3), "istft_bwd": round(frac(out_bytes + spec_bytes, t_ib), 3)}}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del plan, batch, spec
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
