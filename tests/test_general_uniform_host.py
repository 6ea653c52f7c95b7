"""Chip-filling uniform batches, every optimiser step and the output of the general route (key general_geometry; DESIGN.md
sections 31 and 33), host side: the table of cases that tests/test_gpu_general_uniform.py runs on the device, the seeds of
its compared clips, and the two facts that module relies on and a CPU can check.

Cases (geometry of tests/test_gpu_general_geometry.py, samples per clip, clips): the smallest shapes that still reach each
kernel kind det_plan (csrc/capi.hip) gives a batch of equal-length clips.

    UA  G1  256 / 64 / 256 hann, 16 kHz, 500-4000 Hz     stride   64  n =  4000  T =  63  pooled 31  1 row group   B = 192
    UB  G1                                               stride   64  n = 11000  T = 172  pooled 86  3 row groups  B = 193
    UC  G2  512 / 200 / 400 hamming, 16 kHz, 500-4000 Hz stride  128  n = 16000  T =  81  pooled 40  2 row groups  B = 192
    UD  G4  2048 / 512 / 2048 hann, 44.1 kHz, 500-4000   stride  192  n = 44100  T =  87  pooled 43  2 row groups  B = 193
    UE  G5  4096 / 1024 / 4096 hann, 16 kHz, 0-8000 Hz   stride 2112  n = 16000  T =  16  pooled  8  1 row group   B = 192
    UF  G2  as UC                                        stride  128  n = 16000  T =  81  pooled 40  2 row groups  B =  32

Slot i of a case holds make_clip(FILL_SEED + i, n), except the compared slots 0, 1, B/2 - 1, B/2 and B - 2, which hold the
clips of SEEDS, and slot B - 1, which repeats slot 0's clip and payload.

Kink rule.  The loss is not differentiable where a LeakyReLU argument of the detector is 0, and within float32 rounding of 0
the sign, and with it a finite part of the gradient, is decided by rounding in any implementation.  The compared seeds are
therefore chosen here, as tests/test_gpu_loop_run_lengths.py chooses its own: per case the first seeds from SEED_START on
whose clip keeps every LeakyReLU argument at least KINK = 8e-6 from 0 in the float64 and in the float32 restatement.
test_compared_seeds_keep_their_distance recomputes every kept seed's distance, so the device test needs no kink exception
and has none.  Smallest distance of each kept seed in either precision, and the seeds rejected before it with theirs:
    UA: 501 (1.9e-05; 500 at 6.5e-07); 504 (1.2e-05; 502 at 4.9e-06, 503 at 3.1e-06); 505 (2.9e-05); 506 (1.1e-05);
      507 (4.7e-05)
    UB: 503 (8.8e-06; 500 at 4.4e-06, 501 at 2.2e-06, 502 at 1.8e-06); 505 (1.1e-05; 504 at 7.7e-07); 506 (1.2e-05);
      507 (1.5e-05); 515 (1.8e-05; 508 at 7.5e-06, 509 at 3.5e-07, 510 at 4.9e-07, 511 at 1.9e-06, 512 at 2.4e-06,
      513 at 4.0e-07, 514 at 1.9e-06)
    UC: 500 (2.8e-05); 501 (1.4e-05); 502 (8.3e-06); 503 (1.2e-05); 507 (1.8e-05; 504 at 4.4e-07, 505 at 3.6e-06,
      506 at 1.7e-06)
    UD: 502 (1.9e-05; 500 at 2.9e-06, 501 at 2.2e-06); 503 (1.0e-05); 504 (1.8e-05); 507 (3.5e-05; 505 at 1.8e-06,
      506 at 6.0e-06); 510 (9.1e-06; 508 at 3.7e-06, 509 at 7.6e-06)
    UE: 501 (1.1e-05; 500 at 4.7e-06); 502 (3.1e-05); 503 (2.6e-05); 504 (4.9e-05); 505 (6.7e-05)
    UF: UC's clips
"""
import numpy as np
import pytest
import torch

from conftest import make_clip
from oracle import aware_oracle as O
from test_general_geometry_host import GeneralLoop
from test_gpu_general_geometry import GEOM, STRIDE, lengths_of, trivial
from test_gpu_kernels import _min_kink_distance

KINK = 8e-6
SEED_START = 500
FILL_SEED = 1000
# case: geometry, samples per clip, clips, (frames, pooled rows, 32-row groups) per clip
CASES = {
    "UA": ("G1", 4000, 192, (63, 31, 1)),
    "UB": ("G1", 11000, 193, (172, 86, 3)),
    "UC": ("G2", 16000, 192, (81, 40, 2)),
    "UD": ("G4", 44100, 193, (87, 43, 2)),
    "UE": ("G5", 16000, 192, (16, 8, 1)),
    "UF": ("G2", 16000, 32, (81, 40, 2)),
}
# the clip seeds of slots 0, 1, B/2 - 1, B/2, B - 2 (slot B - 1 repeats slot 0); UF has UC's geometry and length, so its seeds
SEEDS = {
    "UA": [501, 504, 505, 506, 507],
    "UB": [503, 505, 506, 507, 515],
    "UC": [500, 501, 502, 503, 507],
    "UD": [502, 503, 504, 507, 510],
    "UE": [501, 502, 503, 504, 505],
    "UF": [500, 501, 502, 503, 507],
}
# every step, with steps that do not improve (part B of the device module)
STEP_LR, STEP_COUNT, RAGGED_SEED = 3.0, 10, 300
# ... and the registry optimiser of that part: the rate reaches 0 at step 3 and returns
REGISTRY = ("adam", {"lr": 0.5}, "cosine_annealing", {"T_max": 3})


def compared_slots(B):
    return [0, 1, B // 2 - 1, B // 2, B - 2, B - 1]


def slot_seeds(name):
    """The make_clip seed of every slot of a case."""
    _, _, B, _ = CASES[name]
    seeds = [FILL_SEED + i for i in range(B)]
    for slot, s in zip(compared_slots(B)[:5], SEEDS[name]):
        seeds[slot] = s
    seeds[B - 1] = seeds[0]
    return seeds


def general_loop(geom, dtype=torch.float64, **kw):
    n_fft, hop, win, window, sr, band, _ = GEOM[geom]
    return GeneralLoop(n_fft, hop, win, window, sr, band, dtype=dtype, **kw)


_LOOPS = {}


def kink_distance(geom, clip):
    """Smallest |u| over the LeakyReLU arguments of the clip's first loop body, in the float64 and the float32 restatement."""
    out = []
    for dtype in (torch.float64, torch.float32):
        if (geom, dtype) not in _LOOPS:
            _LOOPS[geom, dtype] = general_loop(geom, dtype)
        loop = _LOOPS[geom, dtype]
        with torch.no_grad():
            mag0, phase = loop.analyse(torch.as_tensor(clip, dtype=dtype)[None])
        out.append(_min_kink_distance(loop, mag0, phase))
    return tuple(out)


def choose_seeds(geom, n, count=5, start=SEED_START):
    """The rule of the module docstring: (kept seeds, {seed: (float64 distance, float32 distance)} of every seed tried)."""
    kept, tried, s = [], {}, start
    while len(kept) < count:
        tried[s] = kink_distance(geom, make_clip(s, n)[0])
        if min(tried[s]) >= KINK:
            kept.append(s)
        s += 1
    return kept, tried


def step_losses(loop, clip, wm, lr=STEP_LR, steps=STEP_COUNT):
    """Per-step losses of one clip under the card's NAdam at learning rate `lr`: GeneralLoop.embed's loop body with
    O.nadam_schedule(steps, lr=lr) (GeneralLoop.embed itself is fixed at the card's 0.1)."""
    audio = torch.as_tensor(clip, dtype=loop.dtype)[None]
    target = torch.as_tensor(wm, dtype=loop.dtype)[None]
    with torch.no_grad():
        mag0, phase = loop.analyse(audio)
        c0 = mag0[:, loop.band].clone()
        lo, hi = loop.bounds(c0)
    c = c0.clone().requires_grad_(True)
    m, v = torch.zeros_like(c0), torch.zeros_like(c0)
    cg, cm, bc2 = O.nadam_schedule(steps, lr=lr)
    losses = []
    for it in range(steps):
        c.grad = None
        loss, _ = loop.forward_loss(c, mag0, phase, target)
        loss.sum().backward()
        with torch.no_grad():
            O.nadam_step(c.data, c.grad, m, v, cg[it], cm[it], bc2[it])
            c.data = torch.clamp(c.data, lo, hi)
        losses.append(float(loss.detach()[0]))
    return losses


def improvements(losses):
    """losses [steps, clips] -> bool [steps, clips]: the step's loss is below every earlier one (strict, as the loop's best
    snapshot decides it)."""
    losses = np.asarray(losses, dtype=np.float64)
    best = np.minimum.accumulate(np.vstack([np.full((1, losses.shape[1]), np.inf), losses]), axis=0)[:-1]
    return losses < best


def check_non_improvement(losses, who):
    """The condition part B needs of a trajectory: some step >= 1 at which one clip does not improve while another does, and
    at least three (clip, step) pairs without improvement in all.  Returns the improvement table."""
    imp = improvements(losses)
    assert imp[0].all(), who                                            # every loss is below inf
    mixed = [s for s in range(1, imp.shape[0]) if imp[s].any() and not imp[s].all()]
    assert mixed, (who, "no step at which one clip improves and another does not")
    assert int((~imp).sum()) >= 3, (who, int((~imp).sum()))
    return imp


def test_case_table():
    """Frames, pooled rows, row groups and band stride of every case are what the table says, every case's clip count is on
    the side of det_plan's thresholds the table means (kMelFrontMinClips = 192 from the source), the compared slots are six
    different ones and no filler seed is a compared seed."""
    from aware_amd import runtime as rt
    from aware_amd.utils.audio import band_bins
    from test_gpu_mel_norm_bits import constant
    min_clips = constant("capi.hip", "kMelFrontMinClips")
    for name, (geom, n, B, (T, pooled, groups)) in CASES.items():
        n_fft, hop, win, window, sr, band, _ = GEOM[geom]
        assert n > n_fft // 2 and rt.nola_ok(n_fft, hop, win, window, n)
        assert (1 + n // hop, (1 + n // hop) // 2, ((1 + n // hop) // 2 + 31) // 32) == (T, pooled, groups), name
        assert 2 <= T <= 192 and 1 <= groups <= 4                       # mel_front_x3_supported, clip_tile_groups
        lo, hi = band_bins(sr, n_fft, band)
        assert rt.general_band_stride(hi - lo + 1) == STRIDE[geom] != 256
        assert (B >= min_clips) == (name != "UF")
        slots = compared_slots(B)
        assert len(set(slots)) == 6 and slots == sorted(slots) and slots[-1] == B - 1
        seeds = slot_seeds(name)
        assert len(seeds) == B and seeds[B - 1] == seeds[0] and len(set(seeds[:-1])) == B - 1
    assert {CASES[k][2] for k in ("UB", "UD")} == {min_clips + 1} and SEEDS["UF"] == SEEDS["UC"]


@pytest.mark.parametrize("name", ["UA", "UB", "UC", "UD", "UE"])
def test_compared_seeds_keep_their_distance(name):
    """Every compared clip keeps every LeakyReLU argument at least KINK from its kink in the float64 and in the float32
    restatement (UF compares UC's clips)."""
    geom, n, _, _ = CASES[name]
    assert len(SEEDS[name]) == 5 and len(set(SEEDS[name])) == 5 and min(SEEDS[name]) >= SEED_START
    for s in SEEDS[name]:
        d64, d32 = kink_distance(geom, make_clip(s, n)[0])
        print(f"{name} seed {s}: nearest LeakyReLU kink {d64:.1e} (float64) / {d32:.1e} (float32)")
        assert min(d64, d32) >= KINK, (name, s, d64, d32)


def test_float32_restatement_has_steps_that_do_not_improve():
    """At lr = 3.0 the float32 restatement's ten-step trajectory on the ragged G2 batch (seeds 300 to 303) has steps at which
    one clip improves and another does not: what makes the device's clip lookup and its conditional best snapshot visible.
    The one-pooled-frame clip has loss 1 throughout and improves at step 0 only."""
    lengths = lengths_of("G2")
    loop = general_loop("G2", torch.float32)
    fast = []
    for i, n in enumerate(lengths):
        if trivial("G2", i):
            fast.append([1.0] * STEP_COUNT)
            continue
        clip, bits = make_clip(RAGGED_SEED + i, n)
        wm = (2 * bits - 1).astype(np.float32)
        fast.append(step_losses(loop, clip, wm))
    fast = np.asarray(fast).T
    imp = check_non_improvement(fast, "float32 restatement, G2 ragged")
    for i in range(len(lengths)):
        print(f"G2 clip {i} (n = {lengths[i]}): losses at lr 3.0 {np.round(fast[:, i], 4).tolist()}, no improvement at steps "
              f"{np.flatnonzero(~imp[:, i]).tolist()}")
    short = [i for i in range(len(lengths)) if trivial("G2", i)]
    assert len(short) == 1 and imp[:, short[0]].tolist() == [True] + [False] * (STEP_COUNT - 1)
    moving = [i for i in range(len(lengths)) if i not in short]
    assert int((~imp[:, moving]).sum()) >= 3                            # ... not counting the clip that never moves


@pytest.mark.filterwarnings("ignore:Converting a tensor with requires_grad=True to a scalar")     # embed_registry's float(loss)
def test_float32_restatement_of_the_registry_case_has_steps_that_do_not_improve():
    """Adam at 0.5 under cosine annealing with T_max = 3, ten steps, the ragged G2 batch: in the float32 restatement's
    torch.optim loop the three clips that move have eight (clip, step) pairs without improvement (step 4 for every clip: the
    rate is 0 at step 3, so the loss repeats).  With T_max = 10 there is one such pair in all, clip 1 at step 2."""
    name, params, sched, sparams = REGISTRY
    n_fft, hop, win, window, sr, band, _ = GEOM["G2"]
    lengths = lengths_of("G2")
    moving = [i for i in range(len(lengths)) if not trivial("G2", i)]
    losses = []
    for i in moving:
        clip, bits = make_clip(RAGGED_SEED + i, lengths[i])
        ref = []
        GeneralLoop(n_fft, hop, win, window, sr, band, num_iterations=STEP_COUNT, optimizer=name, optimizer_params=params,
                    scheduler=sched, scheduler_params=sparams).embed_registry(
            clip[None], (2 * bits - 1).astype(np.float32)[None], record=lambda it, l, lr: ref.append(l))
        losses.append(ref)
    imp = check_non_improvement(np.asarray(losses).T, "float32 restatement, Adam under cosine annealing")
    for k, i in enumerate(moving):
        print(f"G2 clip {i}: losses {np.round(losses[k], 4).tolist()}, no improvement at steps {np.flatnonzero(~imp[:, k]).tolist()}")
    assert not imp[4].any() and int((~imp).sum()) >= 3
