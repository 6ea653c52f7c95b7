"""The conv block tail's kernels (norm_act_{fwd,bwd}_kernel) at a user's sizes, for an A/B of two builds of the library.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/norm_act_ab.py run r32|r80|mem
    python tools/norm_act_ab.py table LABEL=DIR [LABEL=DIR ...]

`run`: the model card's net through aware_detector_train_gradients (the f32 pipe: on a ragged batch every block is
Conv::Plain, so every block's tail is one of these kernels) on 256 clips of seeded lengths: r32 1-2 s (register form R = 32),
r80 3-8 s (R = 80), mem 8-10.5 s (from memory; the longest clip has 328 pooled frames).  3 calls to warm up, 10 more.
AWARE_HIP_LIB selects the build.
`table`: median duration per launch (us) of the tail kernels in each DIR's kernel trace, per kernel and channel count (the
grid's x size / 256 * 64), with the launches counted."""
import csv
import glob
import os
import re
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SECONDS = {"r32": (1.0, 2.0), "r80": (3.0, 8.0), "mem": (8.0, 10.5)}


def run(workload):
    import numpy as np
    import torch
    from aware_amd import runtime as rt
    from aware_amd.detection import AWAREDetectorNet
    from aware_amd.utils.audio import default_plan
    lo, hi = SECONDS[workload]
    rng = np.random.default_rng(8)
    lengths = [int(v) for v in rng.integers(int(lo * 16000), int(hi * 16000), 256)]
    lengths[-1] = int(hi * 16000)
    plan = default_plan()
    dev = AWAREDetectorNet().device_weights(plan)
    batch = rt.Batch(lengths)
    mag = torch.zeros((batch.total_frames, rt.SPEC_STRIDE), device="cuda")
    mag[:, :225] = 0.3 * torch.randn((batch.total_frames, 225), generator=torch.Generator("cuda").manual_seed(8), device="cuda").abs()
    target = torch.from_numpy(np.where(rng.integers(0, 2, (256, 20)) > 0, 1.0, -1.0).astype(np.float32)).cuda()
    for _ in range(13):
        _, losses, _, _ = rt.detector_train_gradients(plan, dev, batch, mag, target)
    torch.cuda.synchronize()
    print(workload, "longest clip", max(batch.frames) // 2, "pooled frames; mean loss", float(losses.mean()))


def medians(d):
    """{(kernel, channels): (median us, launches)} of the tail kernels in the kernel trace under d."""
    groups = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                name = re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void aware::", "").replace("aware::", "")
                if "norm_act" not in name and "in_lrelu" not in name:
                    continue
                key = (name, int(r["Grid_Size_X"]) // 256 * 64)
                groups.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: (statistics.median(v), len(v)) for k, v in groups.items()}


def table(args):
    for a in args:
        label, d = a.split("=", 1)
        for (name, ch), (med, n) in sorted(medians(d).items()):
            print(f"{label:10s} {name:44s} C {ch:5d}  median {med:9.2f} us  {n:4d} launches")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        table(sys.argv[2:])
