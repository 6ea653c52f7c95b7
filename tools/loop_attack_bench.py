"""Attack-aware embedding (DESIGN.md sections 15 to 21): what a chain of loop attacks costs per iteration, and what it buys.

  (a) config-3 batch (256 x 3 s): per-iteration time of the graph-replayed loop with no chain, noise only, suppression only,
      both, reverberation only, reverberation followed by noise, speed change only, speed change followed by noise, time stretch only, time stretch followed by a speed change, pitch shift only, the phase vocoder with both modes, sample deletion only and sample deletion between a suppression and noise, from device events over --steps steps (>= 200) after a warm-up, the variants alternating in one process
      (--rounds rounds; the median over rounds is reported; --variants a,b,c measures those and `none` only);
  (a') --sync n: the time of AWAREDetector.detect_batch's device work on that batch, trimmed by 256 samples, plain and with
      sync_search = n (median of 10 calls after a warm-up);
  (b) the BER table at that size: 400-step embeddings without a chain, with noise at 10 dB and with 0.5 s suppression
      (prob 0.75), with the reverberation, the reverberation followed by noise and the speed change in the loop, then clean /
      Gaussian noise at 10 and 5 dB / 0.5 s and 0.3 s zeroed / reverberation of rt60 0.1 and 0.3 s / an echo of 100 ms x 0.7 /
      polyphase resampling at 101/100, 21/20, 20/21, 11/10 and 10/11 (--no-ber skips it).
`--mixture a,b` adds the named attack mixtures of MIXTURES and each of their chains alone to (a), so that
a mixture's iteration reads against the weighted mean and the sum of its chains.  `--dump FILE` does none of the above: it runs
20 iterations of a kind-0/1 chain and of a pitch-shift chain on ten 1 s clips and writes the sha256 of the coefficients, the best
coefficients, the losses and the finished waveform, the record a change to the loop is compared against.
`--envelope` adds the chains of ENVELOPE_VARIANTS, which hold the gain envelope, to (a); `--variants` may
name them too.
`--filter` adds the chains of FILTER_VARIANTS, which hold the band filter, in the same way.  `--fir` does
none of the above: it times the FIR kernel alone (aware_band_filter) on the batch against aware_convolve fed the same 255 taps,
from device events, 20 calls each after a warm-up (under rocprofv3 --kernel-trace --stats the two show per kernel).
`--excerpt` adds the chains of EXCERPT_VARIANTS, which hold the tiled excerpt, in the same way.
`--warp` adds the chains of WARP_VARIANTS, which hold the time warp, in the same way.
`--shift` adds the chains of SHIFT_VARIANTS, which hold the frequency shift, in the same way; their
`shift_p1` and `filter_p1` fire on every clip, for a per-kernel comparison of the two FIR kernels inside the loop.  `--ssb` does
none of the above: it times the frequency shift's kernel alone (aware_frequency_shift, forward and adjoint) against the band
filter's (aware_band_filter) on the batch, the three alternating, from device events around windows of 50 launches on buffers
made beforehand: the median of three windows each.
`--only-loop` runs a few steps of every variant and nothing else, for a per-kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/loop_attack_bench.py --only-loop)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aware_amd import attacks as A
from aware_amd import runtime as rt
from aware_amd.utils.models import load

VARIANTS = {
    "none": None,
    "noise": [{"kind": "gaussian_noise", "snr_db": 10.0}],
    "suppression": [{"kind": "sample_suppression", "seconds": 0.5, "prob": 0.75}],
    "both": [{"kind": "sample_suppression", "seconds": 0.3}, {"kind": "gaussian_noise", "snr_db": 10.0}],
    "reverb": [{"kind": "reverberation", "rt60": [0.1, 0.5], "drr_db": -3.0, "prob": 0.75}],
    "reverb_noise": [{"kind": "reverberation", "rt60": [0.1, 0.5], "drr_db": -3.0, "prob": 0.75},
                     {"kind": "gaussian_noise", "snr_db": 10.0}],
    "speed": [{"kind": "speed_change", "cents": 200.0, "prob": 0.75}],
    "speed_noise": [{"kind": "speed_change", "cents": 200.0, "prob": 0.75}, {"kind": "gaussian_noise", "snr_db": 10.0}],
    "stretch": [{"kind": "time_stretch", "rate": [0.85, 1.15], "prob": 0.75}],
    "stretch_speed": [{"kind": "time_stretch", "rate": [0.85, 1.15], "prob": 0.75},
                      {"kind": "speed_change", "cents": 100.0, "prob": 0.75}],
    "pitch": [{"kind": "pitch_shift", "cents": 100.0, "prob": 0.75}],
    "phase_vocoder": [{"kind": "phase_vocoder", "rate": [0.85, 1.15], "cents": 150.0, "prob": 0.9}],
    "delete": [{"kind": "delete_samples", "seconds": 0.032, "prob": 0.75}],
    "suppression_delete_noise": [{"kind": "sample_suppression", "seconds": 0.3}, {"kind": "delete_samples", "seconds": [0.01, 0.2], "at": "anywhere", "prob": 0.75},
                                 {"kind": "gaussian_noise", "snr_db": 10.0}],
}

# The chains with a gain envelope (chain kind 8) live in a table of their own: the recorded fixtures of the loop's chains
# (tests/golden/loop_chains_sha256.json) key on VARIANTS, names and count.
ENVELOPE_VARIANTS = {
    "envelope": [{"kind": "gain_envelope", "period": [0.05, 0.5], "prob": 0.75}],
    "envelope_noise": [{"kind": "gain_envelope", "period": [0.05, 0.5], "prob": 0.75}, {"kind": "gaussian_noise", "snr_db": 10.0}],
    "envelope_64": [{"kind": "gain_envelope", "period": 0.004}],
    "envelope_reverb_envelope": [{"kind": "gain_envelope", "period": [0.05, 0.5], "prob": 0.75},
                                 {"kind": "reverberation", "rt60": [0.1, 0.5], "drr_db": -3.0, "prob": 0.75},
                                 {"kind": "gain_envelope", "period": 0.25, "floor": 0.25}],
}

# The chains with a band filter (chain kind 9), in a table of their own for the same reason.
FILTER_VARIANTS = {
    "filter": [{"kind": "band_filter", "response": ["lowpass", "highpass", "bandpass", "bandstop"], "freq": [600.0, 3800.0], "prob": 0.75}],
    "filter_noise": [{"kind": "band_filter", "response": ["lowpass", "highpass", "bandpass", "bandstop"], "freq": [600.0, 3800.0], "prob": 0.75},
                     {"kind": "gaussian_noise", "snr_db": 10.0}],
    "noise_filter": [{"kind": "gaussian_noise", "snr_db": 10.0},
                     {"kind": "band_filter", "response": ["lowpass", "highpass", "bandpass", "bandstop"], "freq": [600.0, 3800.0], "prob": 0.75}],
}

# The chains with a tiled excerpt (chain kind 10), in a table of their own for the same reason.
EXCERPT_VARIANTS = {
    "excerpt": [{"kind": "excerpt", "seconds": [0.1875, 0.625], "prob": 0.75}],
    "excerpt_noise": [{"kind": "excerpt", "seconds": [0.1875, 0.625], "prob": 0.75}, {"kind": "gaussian_noise", "snr_db": 10.0}],
}

# The chains with a time warp (chain kind 11), in a table of their own for the same reason.
WARP_VARIANTS = {
    "warp": [{"kind": "time_warp", "depth": 0.04, "period": [0.032, 0.512], "prob": 0.75}],
    "warp_noise": [{"kind": "time_warp", "depth": 0.04, "period": [0.032, 0.512], "prob": 0.75}, {"kind": "gaussian_noise", "snr_db": 10.0}],
}

# The chains with a frequency shift (chain kind 12), in a table of their own for the same reason; the two that always fire are
# what a kernel trace compares.
SHIFT_VARIANTS = {
    "shift": [{"kind": "frequency_shift", "hz": 120.0, "prob": 0.75}],
    "shift_noise": [{"kind": "frequency_shift", "hz": 120.0, "prob": 0.75}, {"kind": "gaussian_noise", "snr_db": 10.0}],
    "shift_p1": [{"kind": "frequency_shift", "hz": 120.0}],
    "filter_p1": [{"kind": "band_filter", "response": ["lowpass", "highpass", "bandpass", "bandstop"], "freq": [600.0, 3800.0]}],
}


MIXTURES = {
    "four_families": [
        {"weight": 0.2, "chain": [{"kind": "sample_suppression", "seconds": 0.3, "prob": 0.75}, {"kind": "gaussian_noise", "snr_db": 10.0}]},
        {"weight": 0.2, "chain": [{"kind": "reverberation", "rt60": [0.1, 0.5], "drr_db": -3.0, "prob": 0.75},
                                  {"kind": "gaussian_noise", "snr_db": 20.0}]},
        {"weight": 0.2, "chain": [{"kind": "phase_vocoder", "rate": [0.85, 1.15], "cents": 150.0, "prob": 0.9}]},
        {"weight": 0.2, "chain": [{"kind": "delete_samples", "seconds": [0.01, 0.2], "at": "anywhere", "prob": 0.75},
                                  {"kind": "gaussian_noise", "snr_db": 10.0}]},
    ],
    "tempo_pitch": [
        {"weight": 0.4, "chain": [{"kind": "time_stretch", "rate": [0.85, 1.15]}, {"kind": "speed_change", "cents": 200.0}]},
        {"weight": 0.3, "chain": [{"kind": "pitch_shift", "cents": 150.0}]},
        {"weight": 0.3, "chain": [{"kind": "speed_change", "cents": 200.0}, {"kind": "gaussian_noise", "snr_db": 10.0}]},
    ],
}


def dump(emb, path, names=("both", "pitch"), lengths=None, iters=20):
    """sha256 of what `iters` iterations of a handle leave, per entry of `names` (a chain of VARIANTS or FILTER_VARIANTS, or a mixture of MIXTURES,
    which is set through emb.loop_attack_mixture), on ten 1 s clips or a ragged batch of `lengths`; written to `path` unless it
    is empty."""
    import hashlib
    lengths = [16000] * 10 if lengths is None else [int(n) for n in lengths]
    g = torch.Generator(device="cuda").manual_seed(11)
    audio = 0.1 * torch.randn(sum(lengths), generator=g, device="cuda")
    target = torch.randint(0, 2, (len(lengths), 20), generator=g, device="cuda").float() * 2 - 1
    batch = rt.Batch(lengths)
    out = {}
    chains = {**VARIANTS, **FILTER_VARIANTS}
    for name in names:
        emb.loop_attacks, emb.loop_attack_mixture = (chains[name], []) if name in chains else ([], MIXTURES[name])
        sess = emb.start_session(batch, 16000)
        sess.begin(audio, target)
        sess.iterate(iters)
        parts = {"coef": sess.coef, "best": sess.best_coef, "loss": sess.loss, "best_loss": sess.best_loss, "out": sess.finish(None)}
        out[name] = {k: hashlib.sha256(v.detach().cpu().numpy().tobytes()).hexdigest() for k, v in parts.items()}
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
    return out


def dump_alone(path=""):
    """sha256 of what the stand-alone entries of the loop's stage kernels write, by case name, on two clips of 4099 and 7937
    samples packed back to back (an odd second offset, several workgroups per clip), inputs from numpy with fixed seeds: the
    three resamplers forward and adjoint at same-length and true-length outputs, the sample deletion in both directions, and
    the band filter's four responses with their taps; written to `path` unless it is empty."""
    import hashlib
    from aware_amd.embedding.loop_attacks import speed_length
    lengths = [4099, 7937]
    rng = np.random.default_rng(17)
    x = rt.Ragged.from_list([rng.standard_normal(n).astype(np.float32) for n in lengths])
    sha = lambda t: hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()
    out = {}
    for name, fn, ms in (("speed_change", rt.speed_change, (-13520, 17034, -1, 0, 1, 3000)),
                         ("pitch_shift_ola", rt.pitch_shift_ola, (-13520, 17034, -1, 0, 1, 3000)),
                         ("stretch_ola", rt.stretch_ola, (-16384, 21845, -1, 0, 1, 3000))):
        for m in ms:
            for which, z_len in (("same", lengths), ("true", [speed_length(n, m) for n in lengths])):
                g = rt.Ragged.from_list([np.random.default_rng(m % 1000 + b).standard_normal(n).astype(np.float32) for b, n in enumerate(z_len)])
                out[f"{name}/m={m}/{which}/forward"] = sha(fn(x, m, out_lengths=z_len).data)
                out[f"{name}/m={m}/{which}/adjoint"] = sha(fn(g, m, adjoint=True, out_lengths=lengths).data)
    for start, k in (([0, 0], 0), ([0, 0], 512), ([1000, 1000], 333), ([n - 7 for n in lengths], 7)):
        for adjoint in (False, True):
            out[f"delete_samples/start={start[0]}/k={k}/{'adjoint' if adjoint else 'forward'}"] = sha(rt.delete_samples(x, start, k, adjoint=adjoint).data)
    for response in (1, 2, 4, 8):
        z, taps = rt.band_filter(x, response, 2458, 15565, return_taps=True)
        out[f"band_filter/response={response}/out"], out[f"band_filter/response={response}/taps"] = sha(z.data), sha(taps)
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
    return out


def sync_timing(det, audio, B, n, views):
    """us per call of the plain detection and of the offset search over `views` views, on the batch trimmed by 256 samples."""
    from aware_amd.detection import sync
    m = n - 256
    flat = audio.view(B, n)[:, 256:].contiguous().view(-1)
    plan = det._plan(16000)
    dw = det.detection_net.device_weights(plan)
    plain_batch = rt.Batch([m] * B)
    per = max(1, sync.SYNC_MAX_ROWS // views)
    vlen, voff = sync.sync_views([m] * B, views)
    chunks = [rt.Batch(vlen[b0 * views:min(B, b0 + per) * views], [b * m + voff[b * views + j] for b in range(b0, min(B, b0 + per)) for j in range(views)])
              for b0 in range(0, B, per)]

    def plain():
        return rt.detect(plan, dw, plain_batch, flat)

    def search():
        return [rt.sync_select(rt.detect(plan, dw, c, flat), views, det._centre()) for c in chunks]

    out = {}
    for name, fn in (("plain", plain), ("search", search)):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(10):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(1e3 * a.elapsed_time(b))
        out[name] = round(float(np.median(ts)), 1)
    return out


def fir_timing(audio, B, n):
    """us per call of aware_band_filter (a band-pass of 1000 to 3000 Hz on every clip) and of aware_convolve fed its 255 taps."""
    x = rt.Ragged(audio, [n] * B)
    _, taps = rt.band_filter(x, 4, 4096, 12288, return_taps=True)
    h = taps[:, :255].contiguous()
    nh = torch.full((B,), 255, dtype=torch.int32, device="cuda")
    out = {}
    for name, fn in (("band_filter", lambda: rt.band_filter(x, 4, 4096, 12288)), ("convolve_255", lambda: rt.convolve(x, h, nh))):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(20):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(1e3 * a.elapsed_time(b))
        out[name] = round(float(np.median(ts)), 1)
    return out


def ssb_timing(audio, B, n, launches=50, windows=3):
    """us per launch of aware_frequency_shift (forward and adjoint, +50 Hz) and of aware_band_filter (a band-pass of 1000 to
    3000 Hz) on the batch: device events around `launches` launches on buffers made beforehand, the three alternating, the median
    of `windows` windows each and the windows themselves."""
    from aware_amd._lib import load_library
    lib = load_library()
    x = rt.Ragged(audio, [n] * B)
    out = torch.empty_like(audio)
    i32 = lambda v: torch.full((B,), v, dtype=torch.int32, device="cuda")
    d, p0, rs, c1, c2 = i32(3277), i32(0), i32(4), i32(4096), i32(12288)
    ptr = lambda t: t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    head = (ptr(audio), ptr(x.d_off), ptr(x.d_len), B, n)
    calls = {"frequency_shift": lambda: lib.aware_frequency_shift(*head, ptr(d), ptr(p0), 0, ptr(out), st),
             "frequency_shift_adjoint": lambda: lib.aware_frequency_shift(*head, ptr(d), ptr(p0), 1, ptr(out), st),
             "band_filter": lambda: lib.aware_band_filter(*head, ptr(rs), ptr(c1), ptr(c2), ptr(out), None, st)}
    for fn in calls.values():
        for _ in range(5):
            assert fn() == 0
    ts = {name: [] for name in calls}
    for _ in range(windows):
        for name, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            b.synchronize()
            ts[name].append(round(1e3 * a.elapsed_time(b) / launches, 2))
    return {name: {"median": float(np.median(v)), "windows": v} for name, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--steps", type=int, default=208)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-ber", action="store_true")
    ap.add_argument("--only-loop", action="store_true")
    ap.add_argument("--variants", default="")
    ap.add_argument("--sync", type=int, default=0)
    ap.add_argument("--mixture", default="")
    ap.add_argument("--dump", default="")
    ap.add_argument("--envelope", action="store_true")
    ap.add_argument("--filter", action="store_true")
    ap.add_argument("--fir", action="store_true")
    ap.add_argument("--excerpt", action="store_true")
    ap.add_argument("--warp", action="store_true")
    ap.add_argument("--shift", action="store_true")
    ap.add_argument("--ssb", action="store_true")
    args = ap.parse_args()
    B, n = args.clips, int(args.seconds * 16000)
    emb, det = load()
    emb.verbose = False
    if args.dump:
        print(json.dumps(dump(emb, args.dump)))
        return
    g = torch.Generator(device="cuda").manual_seed(3)
    audio = 0.1 * torch.randn(B * n, generator=g, device="cuda")
    bits = torch.randint(0, 2, (B, 20), generator=g, device="cuda")
    target = bits.float() * 2 - 1
    if args.fir:
        t = fir_timing(audio, B, n)
        print(f"FIR of 255 taps on {B} x {n} samples: aware_band_filter {t['band_filter']:.1f} us, aware_convolve {t['convolve_255']:.1f} us "
              f"(host calls included)")
        print(json.dumps({"clips": B, "seconds": args.seconds, "us_per_call": t}))
        return
    if args.ssb:
        t = ssb_timing(audio, B, n)
        for name, v in t.items():
            print(f"{name:24s} {v['median']:8.2f} us per launch on {B} x {n} samples (windows: {v['windows']})")
        print(json.dumps({"clips": B, "seconds": args.seconds, "us_per_launch": t}))
        return
    batch = rt.Batch([n] * B)
    result = {"clips": B, "seconds": args.seconds, "steps": args.steps}

    if args.sync:
        t = sync_timing(det, audio, B, n, args.sync)
        result[f"us_per_detect/plain"], result[f"us_per_detect/sync_search_{args.sync}"] = t["plain"], t["search"]
        print(f"detect: plain {t['plain']:.1f} us, sync_search = {args.sync}: {t['search']:.1f} us ({t['search'] / t['plain']:.2f} x)")
    chosen = {"none"} | {v for v in args.variants.split(",") if v}
    variants = {k: v for k, v in VARIANTS.items() if not args.variants or k in chosen}
    variants.update({k: v for k, v in ENVELOPE_VARIANTS.items() if k in chosen or (args.envelope and not args.variants)})
    variants.update({k: v for k, v in FILTER_VARIANTS.items() if k in chosen or (args.filter and not args.variants)})
    variants.update({k: v for k, v in EXCERPT_VARIANTS.items() if k in chosen or (args.excerpt and not args.variants)})
    variants.update({k: v for k, v in WARP_VARIANTS.items() if k in chosen or (args.warp and not args.variants)})
    variants.update({k: v for k, v in SHIFT_VARIANTS.items() if k in chosen or (args.shift and not args.variants)})
    mixtures = {}
    for m in [v for v in args.mixture.split(",") if v]:
        mixtures[f"mixture:{m}"] = MIXTURES[m]
        for c, entry in enumerate(MIXTURES[m]):
            variants[f"{m}/{c}"] = entry["chain"]
    sessions = {}
    for name, chain in variants.items():
        emb.loop_attacks, emb.loop_attack_mixture = chain or [], []
        sessions[name] = emb.start_session(batch, 16000)
    for name, mix in mixtures.items():
        emb.loop_attacks, emb.loop_attack_mixture = [], mix
        sessions[name] = emb.start_session(batch, 16000)
    emb.loop_attack_mixture = []
    variants = {**variants, **mixtures}
    steps = 16 if args.only_loop else args.steps
    times = {name: [] for name in variants}
    for _ in range(1 if args.only_loop else args.rounds):
        for name, sess in sessions.items():
            sess.begin(audio, target)
            sess.iterate(args.warmup)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            sess.iterate(steps)
            b.record()
            b.synchronize()
            times[name].append(1e3 * a.elapsed_time(b) / steps)
    for name in variants:
        result[f"us_per_iteration/{name}"] = round(float(np.median(times[name])), 2)
        print(f"{name:13s} {np.median(times[name]):8.1f} us per iteration (rounds: {', '.join(f'{t:.1f}' for t in times[name])})")
    base = result["us_per_iteration/none"]
    for name in [v for v in variants if v != "none"]:
        result[f"extra_us/{name}"] = round(result[f"us_per_iteration/{name}"] - base, 2)
    del sessions

    if not (args.no_ber or args.only_loop):
        bits_h = bits.cpu().numpy()

        def ber(x):
            vals = det.detect_device(x.data, rt.Batch(x.lengths), 16000).cpu().numpy()
            return 100.0 * float(((vals > 0).astype(np.int64) != bits_h).mean())

        table = {}
        echo_h = torch.zeros((B, 1601), device="cuda")
        echo_h[:, 0], echo_h[:, 1600] = 1.0, 0.7
        echo_n = torch.full((B,), 1601, dtype=torch.int32, device="cuda")
        for name in ("none", "noise", "suppression", "reverb", "reverb_noise", "speed"):
            emb.loop_attacks = VARIANTS[name] or []
            out, _ = emb.embed_device(audio, batch, 16000, target)
            y = rt.Ragged(torch.cat(batch.unpack_out(out)), batch.out_lengths)
            row = {"clean": ber(y)}
            for snr in (10.0, 5.0):
                row[f"noise_{int(snr)}dB"] = float(np.mean([ber(A.GaussianNoise(snr).apply_batch(y, 16000, seeds=[100000 * s + i for i in range(B)]))
                                                            for s in range(2)]))
            for sec in (0.5, 0.3):
                ny = batch.out_lengths[0]
                starts = [0, (ny - int(sec * 16000)) // 2, ny - int(sec * 16000) - 1]
                row[f"zeroed_{sec}s"] = float(np.mean([ber(A.SampleSupression(sec).apply_batch(y, 16000, starts=[st] * B)) for st in starts]))
            for rt60 in (0.1, 0.3):
                row[f"reverb_{rt60}s"] = float(np.mean([ber(A.Reverberation(rt60, seed=100000 * s + 7).apply_batch(y, 16000))
                                                        for s in range(2)]))
            row["echo_100ms_0.7"] = ber(rt.convolve(y, echo_h, echo_n))
            for up, down in ((101, 100), (21, 20), (20, 21), (11, 10), (10, 11)):
                row[f"polyphase_{up}/{down}"] = ber(A.resample_poly_batch(y, up, down))
            table[name] = {k: round(v, 3) for k, v in row.items()}
            print(f"BER % embedded with {name:12s}: " + ", ".join(f"{k} {v:.2f}" for k, v in row.items()))
        result["ber_percent"] = table
    print(json.dumps(result))


if __name__ == "__main__":
    main()
