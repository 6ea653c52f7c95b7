#!/usr/bin/env python3
"""Headline benchmark: waveform-seconds/sec through embed -> attack -> detect on MI355X.

    python bench.py --gpus N --steps K --warmup W [--workload config3]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A step is one pass of the hot path over one batch of synthetic clips per GPU: 44.1 kHz sigma = 0.1 Gaussian
clips (already resident in HBM) -> polyphase 160/441 -> per-clip 400-iteration embed -> attack stage -> detect ->
bit errors (the loop of the reference's harness, scripts/test.py:52-106).  Workloads are named after
BASELINE.json's configs:
    config3 (default): 256 x 3 s clips per GPU, full attack stack [resample 16k<->44.1k, lowpass, gaussian 20 dB,
                       pcm16] -- the largest single-GPU configuration, the one the metric is quoted on
    config2:           64 x 3 s clips per GPU, clean embed -> detect
    config3_l1:        config3 with the EXTENSION objective push_extremes + 0.05 * mean|c - c0| ("BER + L1" in BASELINE's wording;
                       the reference has no such loss: parity unpinned, specified by the oracle)
    config4:           config3's per-GPU batch on every rank (8 GPUs: 2048 clips); the same code path as config3
    config5:           256 x N clips of seeded 1..10 s with a seeded attack chain per clip drawn from {pcm, resample,
                       lowpass, bandstop, cut, noise}; clips are assigned to ranks by frame count (shard_by_cost)
    stub:              no GPU work at all (CPU tests of the launcher and the collectives)
Clips shard by global index across ranks (weak scaling, no data-path collective); the only collectives are a SUM of
the counters and a MAX of the wall time.  Rank 0 prints ONE JSON line.

`--dump-outputs DIR` writes what rank 0's last timed step returned as .npy files, so that two builds can be compared output for
output on the same seeded inputs.

`--gpus N` without a torchrun environment starts N child ranks itself (one process per GPU) BEFORE anything
touches the GPU; the parent only waits for them.  A world size that differs from --gpus is an error.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s
MFMA_F32_PEAK_TF = 157.3       # MI355X_MICROARCH.md: dense f32-input MFMA peak
MFMA_BF16_PEAK_TF = 2500.0     # MI355X_MICROARCH.md: dense bf16 MFMA peak
MFMA_SUSTAINED_TF = 1247.0     # a tuned dense bf16 GEMM on random data (MI355X_MICROARCH.md, DVFS give-back item 1): what the pipe sustains
WORKLOADS = ["config2", "config3", "config3_l1", "config4", "config5", "train", "stub"]
CONFIG5_KINDS = ["pcm", "resample", "lowpass", "bandstop", "cut", "noise"]


def detector_flops_per_clip_iter(T):
    """fwd + data-grad bwd, as the reference computes it (full K=513 mel)."""
    return 2 * (131328 * T + 3358720 * (T // 2))


def dsp_bytes_per_clip_iter(T):
    """28 500*T - 6 144 algorithmic HBM bytes of the DSP kernels."""
    return 28500 * T - 6144


def log(*a):
    print("[bench]", *a, file=sys.stderr, flush=True)


# ---------------------------------------------------------------------------------------------------
# launcher: one process per GPU
# ---------------------------------------------------------------------------------------------------
def spawn_ranks(n, argv):
    """Start n copies of this script as ranks 0..n-1 (torchrun-style environment) and wait.  Called before any GPU
    call: the parent never initialises HIP.  Returns the worst exit code."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env))
    # poll: on the first rank that exits non-zero, end its siblings (they would otherwise sit in the rendezvous or in a
    # collective until torch's timeout, holding their GPUs) and report the failure.  Fresh children only, never an exec.
    rc = 0
    live = list(procs)
    while live:
        time.sleep(0.2)
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            if code != 0 and rc == 0:
                rc = code
                log(f"rank process {p.pid} exited with {code}: stopping the other ranks")
                for q in live:
                    q.terminate()
        if rc != 0 and live:
            deadline = time.time() + 10
            for q in live:
                try:
                    q.wait(timeout=max(0.1, deadline - time.time()))
                except subprocess.TimeoutExpired:
                    q.kill()
            live = []
    return rc


# ---------------------------------------------------------------------------------------------------
# workloads
# ---------------------------------------------------------------------------------------------------
def config5_plan(per_gpu, world):
    """Seeded description of BASELINE config 5 for `world` ranks: per_gpu*world clips, duration ~ U{1..10 s},
    per-clip chain = random subset (1..3 kinds) in random order of CONFIG5_KINDS.  Returns (seconds[], chains[])."""
    import numpy as np
    rng = np.random.default_rng(20250905)
    n = per_gpu * world
    secs = rng.integers(1, 11, n).tolist()
    chains = []
    for _ in range(n):
        k = int(rng.integers(1, 4))
        chains.append([CONFIG5_KINDS[j] for j in rng.permutation(len(CONFIG5_KINDS))[:k]])
    return secs, chains


def make_attack_of_kind(kind):
    from aware_amd import attacks as A
    return {"pcm": lambda: A.PCMBitDepthConversion(16), "resample": lambda: A.Resample(),
            "lowpass": lambda: A.LowPassFilter(), "bandstop": lambda: A.RandomBandstop(),
            "cut": lambda: A.DeleteSamples(0.1), "noise": lambda: A.GaussianNoise(20.0)}[kind]()


def cpu_baseline(workload):
    """The CPU oracle (a restatement of the reference's torch-CPU path, kind "port") timed on this host on a bounded
    sample of the same workload: SIX 3 s clips as one batch through front end -> embed (all 400 iterations, nothing
    extrapolated) -> attack stack -> detect: 10-15 s of CPU work on the box's 16 cores (the batch lets torch use them: a single clip
    runs at 0.7-0.8 waveform-s/s, six at 1.9)."""
    import numpy as np
    import torch
    from oracle import aware_oracle as O
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    cores = max(1, min(16, avail))      # the GPU box gives one GPU's share of the host: 16 cores
    torch.set_num_threads(cores)
    rng = np.random.default_rng(0)
    nclips = 6
    x44 = (0.1 * rng.standard_normal((nclips, 132300))).astype(np.float32)
    wm = (2 * rng.integers(0, 2, (nclips, 20)) - 1).astype(np.float32)
    # warm-up: thread pools, allocator, filter designs (none of it is the workload)
    w16 = np.stack([O.resample_poly(x, 160, 441) for x in x44]).astype(np.float32)
    O.Embedder(num_iterations=5).embed(w16, wm)
    if workload != "config2":
        O.pcm_bit_depth(O.gaussian_noise_attack(np.asarray(O.lowpass_attack(O.resample_attack(w16[0], 16000, 16000), 16000),
                                                           dtype=np.float32), 20.0, 0), 16)
    t_all = time.time()
    t0 = time.time()
    audio = np.stack([O.resample_poly(x, 160, 441) for x in x44]).astype(np.float32)     # scripts/test.py:60-63
    t_front = time.time() - t0
    emb = O.Embedder(num_iterations=400)
    t0 = time.time()
    y, _ = emb.embed(audio, wm)
    t_emb = time.time() - t0
    ys = [y[i].numpy() for i in range(nclips)]
    t_att = 0.0
    if workload != "config2":
        t0 = time.time()
        for i in range(nclips):
            v = O.resample_attack(ys[i], 16000, 16000)
            v = O.lowpass_attack(v, 16000)
            v = O.gaussian_noise_attack(np.asarray(v, dtype=np.float32), 20.0, i)
            ys[i] = O.pcm_bit_depth(v, 16)
        t_att = time.time() - t0
    t0 = time.time()
    emb.detect_raw(np.stack([np.asarray(v, dtype=np.float32) for v in ys]))
    t_det = time.time() - t0
    full = time.time() - t_all
    return {"value": 3.0 * nclips / full, "unit": "waveform-seconds/sec", "cores": int(torch.get_num_threads()), "kind": "port",
            "sample": f"{nclips} x 3 s clips as one batch, everything timed ({full:.1f} s): front end {t_front*1e3:.0f} ms + 400 embed "
                      f"iterations {t_emb:.2f} s ({t_emb / 400 * 1e3:.1f} ms/iter for the batch) + attack stack {t_att*1e3:.0f} ms + "
                      f"detect {t_det*1e3:.1f} ms; vectorised bounds (no 1.3 s/clip Python loop)"}


def kernel_source_hash():
    """Hash of the kernel sources the library is built from: a stored counter profile is only quoted when it was taken on
    the same kernels."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "aware_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".hpp", ".h")):
            with open(os.path.join(csrc, name), "rb") as f:
                h.update(f.read())
    return h.hexdigest()[:16]


def pmc_traffic_per_launch(per_gpu, kernel_substr):
    """Mean HBM bytes per launch of the dominant kernel from the PMC passes stored under profiles/ (same command, same
    batch; separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE runs -- bench.py cannot collect counters itself).  The CSV's
    first comment line carries the hash of the kernel sources it was measured on: a profile of other kernels is NOT quoted
    (traffic = null).  Returns (bytes, source) or (None, reason)."""
    import csv
    import glob
    cur = kernel_source_hash()
    reason = "no stored counter profile for this batch"
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_hbm_traffic_pmc.csv")), reverse=True):
        with open(path) as f:
            lines = f.readlines()
        tag = next((l.split("kernel_source_hash=")[1].split()[0] for l in lines if l.startswith("#") and "kernel_source_hash=" in l), None)
        rel = os.path.relpath(path, ROOT)
        if tag != cur:
            reason = f"stored profile {rel} was taken on other kernel sources ({tag} != {cur}): not quoted"
            continue
        rows = [r for r in csv.reader(l for l in lines if not l.startswith("#"))][1:]
        sel = [float(r[3]) + float(r[4]) for r in rows if int(r[0]) == per_gpu and kernel_substr in r[1]]
        if len(sel) == 5:
            return sum(sel) / len(sel) * 1048576.0, (f"stored profile {rel} of this workload on these kernel sources (rocprofv3 --pmc "
                                                     "FETCH_SIZE / WRITE_SIZE passes, gfx950 fetch x2 correction); not re-measured in this run")
    return None, reason


DUMP_BUDGET_BYTES = 64_000_000


def dump_outputs(dirpath, arrays):
    """Write {name: tensor} as dirpath/<name>.npy, in the given order: floating arrays keep float32 / float64, integer ones
    become float64 (exact).  All files together stay within DUMP_BUDGET_BYTES: an array that does not fit whole is replaced by
    the elements at a seeded sample of its flat indices (the same indices on every run), which go to <name>_sample_index.npy."""
    import numpy as np
    os.makedirs(dirpath, exist_ok=True)
    left = DUMP_BUDGET_BYTES
    for name, t in arrays.items():
        a = t.detach().cpu().numpy()
        a = a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)
        if a.nbytes + 128 > left:                                # 128: the .npy header
            k = max(0, (left - 256) // (a.itemsize + 8))
            idx = np.sort(np.random.default_rng(0).choice(a.size, size=k, replace=False))
            np.save(os.path.join(dirpath, f"{name}_sample_index.npy"), idx.astype(np.float64))
            a = a.reshape(-1)[idx]
            left -= idx.size * 8 + 128
        np.save(os.path.join(dirpath, f"{name}.npy"), a)
        left -= a.nbytes + 128
    log(f"outputs of the last timed step written to {dirpath} ({DUMP_BUDGET_BYTES - left} bytes)")


def run_stub(args, rank, world):
    """No GPU: the launcher, the barrier and the reductions only (tests/test_bench_launcher.py)."""
    from aware_amd import parallel
    parallel.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.01)
    parallel.barrier()
    wall = time.perf_counter() - t0
    sums, maxes = parallel.reduce_metrics({"seconds": 3.0 * args.steps, "ranks": 1}, {"wall": wall}, device="cpu")
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"metric": "stub", "value": sums["seconds"] / maxes["wall"], "unit": "waveform-seconds/sec",
                          "n_gpus": world, "ranks_seen": int(sums["ranks"]), "steps": args.steps, "warmup": args.warmup,
                          "config": {"workload": "stub"}}))
    return 0


def run_train(args, rank, world):
    """EXTENSION workload (BASELINE north_star: "RCCL all-reduce over xGMI on the embedder/detector gradients"; the reference trains
    nothing, so there is no reference number and no parity to pin): detector training steps on this rank's clips --
    STFT magnitudes, forward + backward INCLUDING the parameter gradients, one all-reduce of the 6.7 MB gradient bucket across
    the ranks (RCCL; the only data-path collective in the repository), Adam on the device, device images of the weights rebuilt."""
    import torch
    from aware_amd import parallel
    from aware_amd._lib import require_gpu
    require_gpu()
    from aware_amd import runtime as rt
    from aware_amd.utils.models import load
    from aware_amd.training import DetectorTrainer
    dev = torch.device("cuda", torch.cuda.current_device())
    per_gpu = args.clips_per_gpu or 256
    n = int(round(args.seconds * 16000))
    g = torch.Generator(device=dev).manual_seed(100 + rank)
    audio = rt.Ragged(0.1 * torch.randn(per_gpu * n, device=dev, generator=g), [n] * per_gpu)
    bits = torch.randint(0, 2, (per_gpu, 20), device=dev, generator=g)
    _, detector = load()
    tr = DetectorTrainer(detector, lr=1e-4)
    for _ in range(args.warmup):
        loss, _ = tr.step(audio, bits)
    torch.cuda.synchronize()
    parallel.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss, vals = tr.step(audio, bits)
    torch.cuda.synchronize()
    parallel.barrier()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"loss": torch.tensor(loss, dtype=torch.float64), "values": vals, "parameters": tr.flat})
    sums, maxes = parallel.reduce_metrics({"seconds": args.steps * per_gpu * args.seconds}, {"wall": wall}, device=dev)
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        parallel.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({
            "metric": "waveform-seconds/sec through one detector training step (EXTENSION; not BASELINE's metric)",
            "value": round(sums["seconds"] / maxes["wall"], 1), "unit": "waveform-seconds/sec", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(maxes["wall"] / args.steps * 1e3, 2), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32 (f32-input MFMA pipe: the parameter gradients are tested against autograd)",
            "data": "synthetic",
            "config": {"workload": f"train: {per_gpu} x {args.seconds:.0f} s clips/GPU @16 kHz, STFT band -> detector forward + backward with "
                                   "weight gradients -> all-reduce (1.68 M parameters) -> Adam -> weight images rebuilt",
                       "clips_per_gpu": per_gpu, "parallelism": f"dp{world} (gradient all-reduce, RCCL)"},
            "loss": round(float(loss), 6), "roofline": None}))
    return 0


DTYPE_NOTE = {
    "f16x2": "f32 accumulation on the 16-bit MFMA pipe; conv-block GEMMs: every f32 operand scaled by a power of two and carried as TWO "
             "binary16 terms (within one f32 ulp of the operand, rms 2^-24.5), 3 partial products, the l_a*l_b term (<= 2^-22) dropped "
             "-- gemm_h2.hip: error level of an f32 dot product (against fp64 at or below the f32-input MFMA kernel's on every "
             "tested shape), not bit-for-bit f32 operands; mel / read-out / small grids: three bf16 terms, exact, 6 products -- "
             "gemm_x3.hip.  exact_pipe = the same workload with the conv blocks on the exact split",
    "bf16x3": "f32 (every detector GEMM on the bf16 MFMA pipe with each f32 operand split exactly into three bf16 terms, 6 partial "
              "products, f32 accumulation -- gemm_x3.hip)",
    "f32": "f32 (f32-input MFMA)",
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="config3", choices=WORKLOADS)
    ap.add_argument("--clips-per-gpu", type=int, default=0)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--conv-pipe", default="f16x2", choices=("f16x2", "bf16x3", "f32"),
                    help="arithmetic of the conv-block GEMMs (aware_amd.runtime.CONV_PIPES); the default also times bf16x3 beside it")
    ap.add_argument("--no-profile", action="store_true", help="skip the per-kernel HIP-event pass (roofline = null)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what rank 0's last timed step returned as DIR/<name>.npy (float32 / float64, at most 64 MB in all)")
    args = ap.parse_args()
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.dump_outputs and args.workload == "stub":
        ap.error("--dump-outputs: the stub workload computes nothing")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # no torchrun environment: become the launcher (nothing has touched the GPU in this process)
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))

    from aware_amd import parallel
    rank, world, local_rank = parallel.init_distributed(cpu_only=args.workload == "stub")
    if world != args.gpus:
        log(f"world size {world} (WORLD_SIZE) differs from --gpus {args.gpus}")
        sys.exit(2)
    # config5's bandstop and cut attacks draw on the host's global generators (the reference's random / np.random): seeded so
    # that the same arguments give the same inputs on every run
    import random
    import numpy as np
    random.seed(20250905)
    np.random.seed(20250905)
    if args.workload == "stub":
        sys.exit(run_stub(args, rank, world))
    if args.workload == "train":
        sys.exit(run_train(args, rank, world))

    import torch
    from aware_amd._lib import require_gpu
    require_gpu()
    from aware_amd import runtime as rt
    from aware_amd.utils.models import load
    from aware_amd.pipeline import WatermarkPipeline, synthetic_clips, synthetic_ragged_clips
    from aware_amd.attacks import config3_attack_stack, resample_poly_batch

    dev = torch.device("cuda", torch.cuda.current_device())
    wl = args.workload
    per_gpu = args.clips_per_gpu or (64 if wl == "config2" else 256)
    attacks = [] if wl == "config2" else config3_attack_stack()
    embedder, detector = load()
    if wl == "config3_l1":
        from aware_amd.embedding.losses import get_loss_fn
        embedder.loss = get_loss_fn("push_extremes_l1", l1_weight=0.05)
    embedder.use_graph = not args.no_graph
    embedder.conv_pipe = args.conv_pipe
    run_kw = {"input_rate": 44100}
    if wl == "config5":
        secs_all, chains_all = config5_plan(per_gpu, world)
        frames = [1 + (-(-s * 44100 * 160 // 441)) // 256 for s in secs_all]
        mine = parallel.shard_by_cost(frames, world)[rank]           # balance the sum of frame counts per rank
        mine.sort(key=lambda i: (-frames[i], i))                     # longest first inside the rank
        secs = [secs_all[i] for i in mine]
        pipe = WatermarkPipeline(embedder, detector, [], sample_rate=16000)
        audio, bits = synthetic_ragged_clips(secs, 44100, seeds=mine, device=dev)
        run_kw["chains_by_kind"] = ([chains_all[i] for i in mine], make_attack_of_kind)
        n16 = [-(-n * 160 // 441) for n in audio.lengths]
        clip_seconds = float(np.mean(secs))
        desc = (f"config5: {len(mine)} clips/GPU of seeded 1..10 s (mean {clip_seconds:.2f} s) @44.1 kHz -> 16 kHz, embed(400 it) -> "
                "seeded chain of 1..3 of {pcm16, resample, lowpass, bandstop, cut 10 %, gaussian 20 dB} per clip -> detect")
    else:
        pipe = WatermarkPipeline(embedder, detector, attacks, sample_rate=16000, attack_mode="chain")
        audio, bits = synthetic_clips(per_gpu, args.seconds, 44100, first_seed=rank * per_gpu, device=dev)
        n16 = [-(-int(round(args.seconds * 44100)) * 160 // 441)] * per_gpu   # clip length after the 44.1k -> 16k front end
        clip_seconds = args.seconds
        if wl == "config2":
            desc = "config2: %d x %.0f s clips/GPU @44.1 kHz -> 16 kHz, clean embed(400 it) -> detect" % (per_gpu, args.seconds)
        else:
            desc = ("%s: %d x %.0f s clips/GPU @44.1 kHz -> 16 kHz, embed(400 it) -> [resample 16k<->44.1k, lowpass, "
                    "gaussian 20 dB, pcm16] -> detect" % (wl if wl != "config3" or world == 1 else "config4 (config3 per GPU)",
                                                          per_gpu, args.seconds))
            if wl == "config3_l1":
                desc += ("; objective push_extremes + 0.05 * mean|c - c0| (EXTENSION for BASELINE's 'BER + L1' -- the reference has no "
                         "such loss: parity unpinned, specified by oracle/aware_oracle.py)")
    pipe.prepare(n16, input_rate=44100)                              # set-up (tables, tile choice, graphs), not a step
    log(f"rank {rank}/{world}: {len(n16)} clips ({sum(audio.lengths) / 44100.0:.0f} waveform-s) resident on {dev}; warm-up x{args.warmup}")
    for _ in range(args.warmup):
        res = pipe.run(audio, bits, **run_kw)
    torch.cuda.synchronize()
    log("timed region starts")
    parallel.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    errs = torch.zeros((), dtype=torch.int64, device=dev)
    clean = torch.zeros((), dtype=torch.int64, device=dev)
    secs_done = 0.0
    for _ in range(args.steps):
        res = pipe.run(audio, bits, **run_kw)
        errs += res.bit_errors
        clean += res.clean_bit_errors
        secs_done += res.seconds
    torch.cuda.synchronize()
    parallel.barrier()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    log(f"timed region done: {wall:.3f} s for {args.steps} steps")
    if args.dump_outputs and rank == 0:
        # before the profile and exact-pipe passes below, which run on the same sessions
        dump_outputs(args.dump_outputs, {
            "bits": res.bits, "values": res.values, "bit_errors": res.bit_errors, "clean_bit_errors": res.clean_bit_errors,
            "watermarked_lengths": torch.tensor(res.watermarked.lengths), "watermarked": res.watermarked.data})
    sums, maxes = parallel.reduce_metrics(
        {"bit_errors": int(errs), "clean_bit_errors": int(clean), "bits": args.steps * len(n16) * 20, "seconds": secs_done},
        {"wall": wall}, device=dev)

    # ---- roofline of the dominant kernel, measured live with HIP events on the launch stream: 3 eager loop bodies
    # through aware_embed_profile on a freshly begun session (the optimiser steps count against num_iterations) ----
    roof = None
    breakdown = {}
    if rank == 0 and not args.no_profile:
        key = next(k for k in pipe._sessions if not (isinstance(k[0], str)))
        batch, sess = pipe._sessions[key]
        x16 = resample_poly_batch(audio, 16000, 44100)
        sess.begin(x16.data, (2 * bits - 1).to(torch.float32))
        n_it = 3
        prof = rt.embed_profile(sess, n_it)
        for kind, ms in prof:
            d = breakdown.setdefault(kind, [0.0, 0])
            d[0] += ms
            d[1] += 1
        rows = sum(t // 2 for t in batch.frames)                 # valid pooled frames of the batch
        ch = embedder.detection_net.channels                     # [128, 512, 1024, 1024, 40]
        gemm_kinds = [k for k in ("gemm_x3_fwd", "gemm_x3_bwd", "gemm_clip_fwd", "gemm_clip_bwd", "gemm_nt") if k in breakdown]
        all_ms = sum(breakdown[k][0] for k in gemm_kinds)
        all_n = sum(breakdown[k][1] for k in gemm_kinds)
        flops_iter = sum(detector_flops_per_clip_iter(t) for t in batch.frames)
        uniform = len(set(batch.frames)) == 1 and batch.frames[0] // 2 <= 128
        # capi.hip (kH2MinGrid, clip_tile_groups, h2_rag): uniform batches from 32 clips on and every ragged batch run their
        # conv blocks on the f16 two-term kernels; smaller uniform batches on the bf16x3 latency kernel
        on_h2 = args.conv_pipe == "f16x2" and "gemm_x3_fwd" in breakdown and (not uniform or len(batch.frames) >= 32)
        if on_h2:
            peak = MFMA_BF16_PEAK_TF / 3.0
            peak_note = ("f32-equivalent peak of the f16 two-term kernel (gemm_h2.hip): dense f16 MFMA peak (2.5 PFLOP/s, the bf16 "
                         "figure) / 3 partial products per f32 multiply-add")
        else:
            peak = MFMA_BF16_PEAK_TF / 6.0
            peak_note = ("f32-equivalent peak of the bf16 three-term kernel (gemm_x3.hip): dense bf16 MFMA peak (2.5 PFLOP/s) / 6 "
                         "partial products per f32 multiply-add")
        if "gemm_x3_fwd" in breakdown:
            # dominant kernel: the conv block / data-gradient GEMM with fused InstanceNorm + LeakyReLU epilogues, 5 launches per
            # iteration: conv0..2 forward (K = 128, 512, 1024) and the data gradients of conv2, conv1 (K = 1024);
            # (the skinny last conv and its data gradient live in the forward epilogue and in the read-out kernels)
            fl = 2.0 * rows * (ch[0] * ch[1] + ch[1] * ch[2] + ch[2] * ch[3]) + 2.0 * rows * (ch[3] * ch[2] + ch[2] * ch[1])
            ms = breakdown["gemm_x3_fwd"][0] + breakdown["gemm_x3_bwd"][0]
            nl = breakdown["gemm_x3_fwd"][1] + breakdown["gemm_x3_bwd"][1]
            big = not uniform or len(batch.frames) >= 32
            kname = (("gemm_clip_h2_kernel" if uniform else "gemm_ragged_h2_kernel") if on_h2 else
                     ("gemm_clip_x3_kernel" if uniform else "gemm_ragged_x3_kernel") if big else "gemm_clip_x3_small_kernel")
            name = f"aware::{kname} (forward epilogue x3, backward epilogue x2 per iteration)"
            if not uniform:
                # the last conv's data gradient of a ragged batch is one more launch of this kind (readout_grad_ragged_x3_kernel,
                # K = 64 on the bf16x3 arithmetic: 2 % of the flops)
                fl += 2.0 * rows * ch[4] * ch[3]
            per_kernel = {kname + " forward": round(breakdown["gemm_x3_fwd"][0] * 1e3 / breakdown["gemm_x3_fwd"][1], 2),
                          kname + " backward": round(breakdown["gemm_x3_bwd"][0] * 1e3 / breakdown["gemm_x3_bwd"][1], 2)}
        else:
            fl, ms, nl = flops_iter, all_ms, all_n
            name = ("aware::gemm_clip_x3_kernel<1,0,8> on 32-row blocks (+ gemm_nt_kernel for shapes it does not serve): "
                    "all detector GEMMs of the iteration, generic path")
            per_kernel = {"gemm_clip_x3_kernel<1,0,8>|gemm_nt_kernel": round(all_ms * 1e3 / all_n, 2)}
        achieved = fl * n_it / (ms * 1e-3) / 1e12
        dsp_kinds = ("synth", "analysis", "synth_adjoint", "analysis_adjoint_nadam")
        dsp_ms = sum(breakdown[k][0] for k in dsp_kinds)
        dsp_bytes = sum(dsp_bytes_per_clip_iter(t) for t in batch.frames) * n_it
        roof = {"bound": "mfma", "kernel": name, "achieved": round(achieved, 2), "peak": round(peak, 1),
                "unit": "TFLOP/s", "frac": round(achieved / peak, 4), "traffic": None, "peak_note": peak_note,
                "frac_of_f32_mfma_peak": round(achieved / MFMA_F32_PEAK_TF, 4),
                "frac_of_six_product_peak": round(achieved / (MFMA_BF16_PEAK_TF / 6.0), 4),
                "frac_of_sustained": round(achieved / (MFMA_SUSTAINED_TF / (3.0 if on_h2 else 6.0)), 4),
                "frac_of_sustained_note": "achieved / (1.247 PFLOP/s / partial products): 1 247 TFLOP/s = what MI355X_MICROARCH.md (DVFS give-back, item 1) gives "
                                          "for a tuned dense 16-bit GEMM on random data (DVFS give-back); this repo's MFMA-only variant "
                                          "of the conv kernel measures 1.18 on finite operands (profiles/r03_gemm_planes_experiment.txt)",
                "frac_note": "frac = achieved / (2.5 PFLOP/s / partial products per multiply-add of the kernel that ran); round 2's "
                             "bf16x3 kernel ran 6 products (peak 416.7, frac 0.45-0.47), the f16 two-term kernel runs 3 (peak 833.3): "
                             "frac_of_six_product_peak relates this run to round 2's denominator",
                "traffic_unit": "bytes/launch", "traffic_source": None,
                "avg_launch_us": round(ms * 1e3 / nl, 2), "launches_timed": nl,
                "timing": "HIP events on the launch stream around every launch of 3 eager iterations (includes the eager "
                          "inter-kernel gap that graph replay does not have); profiles/ holds the kernel trace of the same command",
                "algorithmic_flops_per_launch": fl * n_it / nl, "avg_launch_us_by_kernel": per_kernel,
                "all_detector_gemms": {"achieved": round(flops_iter * n_it / (all_ms * 1e-3) / 1e12, 2), "unit": "TFLOP/s",
                                       "launches_per_iteration": all_n // n_it,
                                       "note": "SURVEY 8(d) algorithmic detector flops / time of every GEMM launch"},
                "dsp_hbm": {"bound": "hbm", "achieved": round(dsp_bytes / (dsp_ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS,
                            "unit": "GB/s", "frac": round(dsp_bytes / (dsp_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                            "avg_launch_us": round(dsp_ms * 1e3 / (4 * n_it), 2),
                            "algorithmic_bytes_per_iteration": dsp_bytes // n_it}}
        if "gemm_x3_fwd" in breakdown and uniform:
            tb, src = pmc_traffic_per_launch(len(batch.frames), "gemm_clip_h2_kernel<3," if on_h2 else "gemm_clip_x3_kernel<3,")
            roof["traffic"], roof["traffic_source"] = (round(tb) if tb is not None else None), src
            # operands of the five launches: A rows (f32) + output rows (f32) + packed weights (2 x f16 or 3 x bf16), and the
            # forward activation re-read by the two backward epilogues
            pairs = [(ch[0], ch[1]), (ch[1], ch[2]), (ch[2], ch[3]), (ch[3], ch[2]), (ch[2], ch[1])]
            wb = 4.0 if on_h2 else 6.0
            alg = sum(4.0 * rows * (k + n) + wb * k * n for k, n in pairs) + 4.0 * rows * (ch[2] + ch[1])
            roof["algorithmic_bytes_per_launch"] = round(alg / 5)
    # ---- the same workload on the EXACT pipe (three bf16 terms, six products), one step on rank 0 at N = 1: the rate a reader
    # who does not accept the two-term split as f32 arithmetic should take ----
    exact = None
    if world == 1 and args.conv_pipe == "f16x2" and not args.no_profile:
        embedder.conv_pipe = "bf16x3"
        pipe2 = WatermarkPipeline(embedder, detector, pipe.attacks, sample_rate=16000, attack_mode=pipe.attack_mode)
        pipe2.prepare(n16, input_rate=44100)
        pipe2.run(audio, bits, **run_kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r2 = pipe2.run(audio, bits, **run_kw)
        e2 = int(r2.bit_errors)
        torch.cuda.synchronize()
        w2 = time.perf_counter() - t0
        exact = {"conv_pipe": "bf16x3", "value": round(r2.seconds / w2, 2), "unit": "waveform-seconds/sec", "steps": 1,
                 "ms_per_step": round(w2 * 1e3, 2), "ber_percent": round(100.0 * e2 / (len(n16) * 20), 4),
                 "note": "same workload, conv blocks on gemm_x3.hip (every f32 operand split exactly into three bf16 terms, six "
                         "partial products, f32 accumulation): bit-level f32 operands"}
        embedder.conv_pipe = args.conv_pipe
        del pipe2
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        parallel.barrier()
        dist.destroy_process_group()
    if rank != 0:
        return
    value = sums["seconds"] / maxes["wall"]
    out = {
        "metric": "waveform-seconds/sec through embed->attack->detect; BER vs reference",
        "value": round(value, 2), "unit": "waveform-seconds/sec", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(maxes["wall"] / args.steps * 1e3, 2), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None,
        "dtype": DTYPE_NOTE[args.conv_pipe],
        "data": "synthetic",
        "config": {"workload": desc, "clips_per_gpu": len(n16), "clip_seconds": clip_seconds,
                   "iterations": embedder.num_iterations,
                   "parallelism": f"dp{world} (shard by clip, no data-path collective)", "hip_graph": not args.no_graph},
        "ber_percent": round(100.0 * sums["bit_errors"] / sums["bits"], 4),
        "ber_percent_clean": round(100.0 * sums["clean_bit_errors"] / sums["bits"], 4),
        "roofline": roof,
        "exact_pipe": exact,
        "kernel_ms_per_iteration": {k: round(v[0] / 3, 4) for k, v in breakdown.items()},
        "kernel_ms_per_iteration_note": "eager launches, HIP-event timed (each figure includes the 2-5 us eager inter-kernel gap; "
                                        "their sum therefore exceeds ms_per_step / iterations, which runs from hipGraphs)",
    }
    if world == 1 and not args.no_cpu_baseline:
        log("timing the CPU oracle on a bounded sample (about 10-30 s)")
        out["cpu_baseline"] = cpu_baseline(wl)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
