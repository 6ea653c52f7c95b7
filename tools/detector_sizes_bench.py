"""Times detectors of other sizes (detection_net_cfg n_mels, num_blocks, n_filters) against the model card's network.

Per detector, 256 clips x 3 s at 16 kHz:
  - one embed iteration: aware_embed_iterate of a recorded graph (16 loop bodies per replay), per-iteration time;
  - aware_detect on the same clips;
  - the workspace the embed session needs.
HIP-event timing, warm-up, median over repetitions.  Prints one JSON line per detector.
    python tools/detector_sizes_bench.py [--reps 10] [--clips 256] [--seconds 3] [--only KEY] [--out FILE]
KEY: card, m40, m64, m200, f_odd, deep10.
`--dump-bits FILE` times nothing: it writes dump_bits(), the sha256 record of the mel stage's kernels that
tests/test_gpu_mel_norm_bits.py compares against (tests/golden/mel_norm_sha256.json).
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

# dump_bits: the card's detector and one mel bank per count of 128-channel groups (13: one partial group, rows of 16 floats;
# 200: a second, partial group; 300: three; 512: four full ones), the small ones with one 64-channel block and 8 bits
BITS_SMALL = dict(num_blocks=1, n_filters=[64], output_length=8)
BITS_DETECTORS = {"card": {}, "m13": dict(n_mels=13, **BITS_SMALL), "m200": dict(n_mels=200, **BITS_SMALL),
                  "m300": dict(n_mels=300, **BITS_SMALL), "m512": dict(n_mels=512, **BITS_SMALL)}
# ragged batches (T = 1 + n // 256 frames).  clip: T = 3, 63, 64, 192 -- the one-workgroup-per-clip kernels up to their limit,
# odd and even T.  chunked: T = 3, 63, 193, 225, 224 -- 32-frame chunks: short clips leave most chunks at once, last chunks of
# one frame (193, 225) and of 32 (224), unpaired last frames
BITS_RAGGED = {"clip": [600, 16000, 16128, 48896], "chunked": [600, 16000, 49152, 57344, 57088]}
# uniform batches of the card's detector that fill the chip: the one-launch mel front kernel and block 0's data gradient with
# the mel backward, at two instantiations each (T = 63 and 161)
BITS_UNIFORM = {"u63": [16000] * 192, "u161": [40960] * 192}
BITS_EMBED = [16000, 12000, 9000]


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


def dump_bits(path=""):
    """sha256 of what the detector's mel stage feeds forward and back, by case: rt.detector_forward's values, and
    rt.detector_backward's values and magnitude gradient for a seeded grad_values, for every detector of BITS_DETECTORS on the
    batches of BITS_RAGGED and for the card's on BITS_UNIFORM; sess.gradient() of a default EmbedSession on BITS_EMBED after
    begin (the clip kernel as the loop calls it, per-clip maxima included).  Every case also records the sha256 of its inputs
    (mel basis, weights, biases, magnitudes, gradient or audio and payload), so that a changed input is told apart from a
    changed kernel.  Inputs come from numpy generators with fixed seeds.  Written to `path` unless it is empty."""
    import hashlib
    from aware_amd import runtime as rt
    from aware_amd.detection import AWAREDetectorNet
    from aware_amd.utils.audio import default_plan
    rt.require_gpu()
    plan = default_plan()

    def sha(*arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest()

    out = {"inputs": {}, "sha256": {}}
    seed = 1000
    for key, kw in BITS_DETECTORS.items():
        net = AWAREDetectorNet(**kw)
        det = net.device_weights(plan)
        for bname, lengths in {**BITS_RAGGED, **(BITS_UNIFORM if key == "card" else {})}.items():
            seed += 1
            rng = np.random.default_rng(seed)
            batch = rt.Batch(lengths)
            z = rng.standard_normal((batch.total_frames, 225, 2))
            rows = np.zeros((batch.total_frames, rt.SPEC_STRIDE), np.float32)
            rows[:, :225] = 0.3 * np.hypot(z[..., 0], z[..., 1])
            gv = rng.standard_normal((batch.B, net.output_length)).astype(np.float32)
            case = f"{key}/{bname}"
            out["inputs"][case] = sha(net.mel_basis, *net.weights, *net.biases, rows, gv)
            mag = torch.from_numpy(rows).cuda()
            fwd = rt.detector_forward(plan, det, batch, mag)
            vals, gmag = rt.detector_backward(plan, det, batch, mag, torch.from_numpy(gv).cuda())
            out["sha256"][case] = {"forward_values": sha(fwd.cpu().numpy()), "backward_values": sha(vals.cpu().numpy()),
                                   "grad_mag": sha(gmag.cpu().numpy())}
    net = AWAREDetectorNet()
    rng = np.random.default_rng(77)
    clips = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in BITS_EMBED]
    wm = np.where(rng.integers(0, 2, (len(BITS_EMBED), net.output_length)) > 0, 1.0, -1.0).astype(np.float32)
    batch = rt.Batch(BITS_EMBED)
    sess = rt.EmbedSession(plan, net.device_weights(plan), batch)
    sess.begin(batch.pack(clips), torch.from_numpy(wm).cuda())
    out["inputs"]["embed"] = sha(net.mel_basis, *net.weights, *net.biases, *clips, wm)
    out["sha256"]["embed"] = {"gradient": sha(sess.gradient().cpu().numpy())}
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--only", default=None, choices=list(SIZES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--dump-bits", default=None, metavar="FILE")
    args = ap.parse_args()
    if args.dump_bits:
        dump_bits(args.dump_bits)
        return
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
