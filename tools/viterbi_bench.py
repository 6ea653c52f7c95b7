"""The Viterbi decoder's launch time: aware_viterbi_decode on `--rows` rows of `--bits` detector
outputs, frames of random messages in Gaussian noise, `--reps` launches between HIP events in `--rounds` rounds after a
warm-up.  One JSON line: microseconds per launch (median, smallest, largest), rows per second, and the bytes the launch has to
move over that time.  Needs the GPU; there is no fallback.

    python tools/viterbi_bench.py --rows 131072 --bits 512 --rate 1/3 --crc 16
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 17)
    ap.add_argument("--bits", type=int, default=512)
    ap.add_argument("--rate", default="1/3")
    ap.add_argument("--crc", type=int, default=16)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()

    import torch
    from aware_amd import runtime as rt
    from aware_amd._lib import require_gpu
    from aware_amd.utils.watermark import fec
    require_gpu()
    R, L = args.rows, args.bits
    n = len(fec.RATES[fec.check_rate(args.rate)])
    k = fec.capacity(L, args.rate, args.crc)
    rng = np.random.default_rng(0)
    sent = rng.integers(0, 2, (R, k))
    inputs = np.concatenate([sent, fec.crc_bits(sent, args.crc), np.zeros((R, fec.TAIL), dtype=np.int64)], axis=1)
    coded = fec.conv_encode(inputs, args.rate)
    values = np.zeros((R, L), dtype=np.float32)
    values[:, :coded.shape[1]] = 2.0 * coded - 1.0
    values += (args.sigma * rng.standard_normal(values.shape)).astype(np.float32)
    dev = torch.from_numpy(values).cuda()

    out = rt.viterbi_decode(dev, 0.0, args.rate, args.crc)           # warm-up, and the figures of merit of the input
    for _ in range(5):
        rt.viterbi_decode(dev, 0.0, args.rate, args.crc)
    torch.cuda.synchronize()
    right = (fec.unpack_bits(out["bits"].cpu().numpy(), k) == sent).all(axis=1)
    us = []
    for _ in range(args.rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            rt.viterbi_decode(dev, 0.0, args.rate, args.crc)
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) / args.reps * 1e3)
    med = float(np.median(us))
    moved = R * (4 * L + 4 * ((L // n + 31) // 32) + 12)           # the row in, the packed bits and three words out
    print(json.dumps({"rows": R, "n_bits": L, "rate": args.rate, "crc": args.crc, "message_bits": k, "sigma": args.sigma,
                      "messages_right": int(right.sum()), "valid": int(out["valid"].sum().item()),
                      "us_per_launch": {"median": round(med, 1), "min": round(min(us), 1), "max": round(max(us), 1)},
                      "rows_per_second": round(R / (med * 1e-6)), "trellis_steps_per_second": round(R * (L // n) / (med * 1e-6)),
                      "bytes_moved": moved, "gbytes_per_second": round(moved / (med * 1e-6) / 1e9, 1)}), flush=True)


if __name__ == "__main__":
    main()
