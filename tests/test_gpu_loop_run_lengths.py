"""The loop chains at every synthesis run length a batch can select.

aware_batch_create picks the hop blocks per workgroup segment (Batch.synth_run) from the batch: 12 for the bench's 256 x 3 s, 4
for every batch of the other tests/test_gpu_loop_*.py modules (tests/test_loop_run_rule_host.py pins that).  At run 4 a segment
is at most 1024 samples, one pass of every 256-thread loop of the loop kernels; this module runs the same chains, with the same
helpers and the same bounds, on batches that select 12, 8 and 6.

Batches: five head clips [18432, 16000, 8000, 24000, 513] (at run 12: whole tiles, ragged last tiles, several segments of 10 to
12 blocks, and the shortest clip the loop takes) followed by about 2040 short filler clips of seeded noise that only move the
rule and are never compared; U12 is uniform (the chip-filling conv kernels), compared at its first, middle and last slot.

Entry parameters are those of the per-kind modules, except where the 513-sample head clip (512 output samples) and the fillers
rule them out: the suppression is test_gpu_loop_filter's 0.02 s (0.3 s is 4800 samples), the deletions keep their `at` modes
with 0.02 s and 0.01 to 0.03 s (the modules' 0.032 s is exactly 512 samples, their 0.2 s is 3200).

Run on the MI355X box:  python -m pytest tests/test_gpu_loop_run_lengths.py -m gpu -q -s"""
import numpy as np
import pytest
import torch

from conftest import make_clip
from loop_support import KINK, LA, NOISE10, O, det_for, mixture_session, oracle_gradient, plan_for, rows, rt, span, weights
# this module is about every kind at once: each kind's entries and its forward check come from the module that owns them
from test_gpu_loop_attacks import check_forward as forward_01
from test_gpu_loop_reverb import check_forward as forward_reverb, reverb
from test_gpu_loop_speed import SPEED, check_forward as forward_speed
from test_gpu_loop_stretch import CHAINS as STRETCH_CHAINS, STRETCH, check_forward as forward_stretch
from test_gpu_loop_pitch import PITCH, check_forward as forward_pitch
from test_gpu_loop_pv import PV_BOTH, check_forward as forward_pv
from test_gpu_loop_delete import ANY, CROP, check_forward as forward_delete
from test_gpu_loop_gain import ENV_SHORT
from test_gpu_loop_filter import BF, SUP, check_forward as forward_filter
from test_loop_run_rule_host import BATCHES, HEAD, expected_synth_run

pytestmark = pytest.mark.gpu

COMPARED = {"R12": [0, 1, 2, 3, 4], "R8": [0, 1, 2, 3, 4], "R6": [0, 1, 2, 3, 4], "U12": [0, 341, 682]}
assert SUP["seconds"] == 0.02 and ENV_SHORT["period"] == 0.004
CHAINS = {
    "noise": [NOISE10], "suppression": [SUP], "reverb": [reverb(2049)], "speed": [SPEED], "stretch": [STRETCH], "pitch": [PITCH],
    "pv": [PV_BOTH], "crop": [dict(CROP, seconds=0.02)], "anywhere": [dict(ANY, seconds=[0.01, 0.03])], "envelope": [ENV_SHORT],
    "filter": [BF], "pair": STRETCH_CHAINS["pair"], "four": [SUP, PITCH, ENV_SHORT, NOISE10],
}
# the kinds with launches of their own between the stage kernels, and the envelope with its per-segment table
SPLIT_AND_ENVELOPE = ["reverb", "speed", "stretch", "pitch", "pv", "crop", "anywhere", "envelope", "filter"]
ATTACK_SEED = {18432: 5, 16000: 7, 8000: 9, 24000: 11, 513: 13}            # per head clip; a filler in slot i draws from 1000 + i

# Clip seeds of the compared clips, chosen on the CPU (oracle only) so that the float64 and the float32 composition both keep every
# LeakyReLU argument of the clip at least KINK = 8e-6 from its kink under the chain and the attack seed above: per chain and
# length the first seed from 80 on that passes, at most twelve tried (every one was found within six).  None: the clip stays in
# the batch (seed 80) for the forward and the bit-for-bit checks and is left out of the gradient check.  That is the 513-sample
# clip under every chain: its attacked signal has 512 samples, and the oracle's torch.stft refuses to reflect-pad a signal that
# is not longer than n_fft / 2, so the composition has no value to compare with.
# Smallest distance of the kept seed in either precision, then the seeds rejected before it with theirs:
#   noise: 18432: 80 (1.4e-05); 16000: 82 (2.7e-05; 80 at 3.6e-06, 81 at 7.1e-06); 8000: 80 (5.4e-05); 24000: 81 (1.9e-05; 80 at
#     2.6e-06)
#   suppression: 18432: 81 (2.0e-05; 80 at 5.4e-07); 16000: 80 (1.1e-05); 8000: 83 (3.9e-05; 80 at 6.6e-06, 81 at 5.1e-06, 82 at
#     1.2e-06); 24000: 84 (1.7e-05; 80 at 5.5e-06, 81 at 2.7e-07, 82 at 4.2e-06, 83 at 2.8e-06)
#   reverb: 18432: 80 (8.2e-05); 16000: 80 (1.4e-05); 8000: 81 (6.1e-05; 80 at 5.0e-06); 24000: 80 (2.2e-05)
#   speed: 18432: 80 (2.0e-05); 16000: 80 (1.7e-05); 8000: 80 (1.6e-05); 24000: 80 (1.6e-05)
#   stretch: 18432: 83 (2.9e-05; 80 at 3.9e-06, 81 at 1.1e-06, 82 at 3.9e-06); 16000: 80 (2.1e-05); 8000: 80 (6.6e-05); 24000:
#     80 (1.6e-05)
#   pitch: 18432: 80 (5.6e-05); 16000: 80 (1.3e-05); 8000: 80 (4.7e-05); 24000: 81 (1.1e-05; 80 at 7.8e-06)
#   pv: 18432: 81 (1.9e-05; 80 at 4.1e-06); 16000: 81 (1.6e-05; 80 at 2.8e-06); 8000: 80 (1.9e-05); 24000: 80 (1.2e-05)
#   crop: 18432: 80 (4.5e-05); 16000: 80 (2.3e-05); 8000: 80 (2.1e-05); 24000: 84 (2.4e-05; 80 at 5.7e-06, 81 at 4.4e-06, 82 at
#     1.9e-06, 83 at 3.6e-07)
#   anywhere: 18432: 82 (1.8e-05; 80 at 4.1e-06, 81 at 1.1e-06); 16000: 80 (1.5e-05); 8000: 80 (6.9e-05); 24000: 80 (3.3e-05)
#   envelope: 18432: 82 (9.9e-06; 80 at 2.6e-06, 81 at 2.7e-06); 16000: 81 (1.7e-05; 80 at 3.1e-06); 8000: 80 (1.9e-05); 24000:
#     85 (9.5e-06; 80 at 1.3e-07, 81 at 1.1e-06, 82 at 2.7e-06, 83 at 1.6e-06, 84 at 7.0e-06)
#   filter: 18432: 82 (1.0e-05; 80 at 5.5e-06, 81 at 4.0e-06); 16000: 84 (1.9e-05; 80 at 8.3e-07, 81 at 1.3e-06, 82 at 7.3e-06,
#     83 at 2.1e-06); 8000: 80 (5.3e-05); 24000: 80 (8.1e-06)
#   pair: 18432: 80 (1.9e-05); 16000: 81 (1.7e-05; 80 at 4.2e-07); 8000: 80 (6.8e-05); 24000: 83 (8.2e-06; 80 at 4.1e-06, 81 at
#     3.4e-06, 82 at 1.0e-06)
#   four: 18432: 81 (1.9e-05; 80 at 4.2e-06); 16000: 80 (1.1e-04); 8000: 81 (2.0e-05; 80 at 6.9e-06); 24000: 82 (1.2e-05; 80 at
#     4.3e-07, 81 at 7.4e-06)
SEEDS = {
    "noise": {18432: 80, 16000: 82, 8000: 80, 24000: 81, 513: None},
    "suppression": {18432: 81, 16000: 80, 8000: 83, 24000: 84, 513: None},
    "reverb": {18432: 80, 16000: 80, 8000: 81, 24000: 80, 513: None},
    "speed": {18432: 80, 16000: 80, 8000: 80, 24000: 80, 513: None},
    "stretch": {18432: 83, 16000: 80, 8000: 80, 24000: 80, 513: None},
    "pitch": {18432: 80, 16000: 80, 8000: 80, 24000: 81, 513: None},
    "pv": {18432: 81, 16000: 81, 8000: 80, 24000: 80, 513: None},
    "crop": {18432: 80, 16000: 80, 8000: 80, 24000: 84, 513: None},
    "anywhere": {18432: 82, 16000: 80, 8000: 80, 24000: 80, 513: None},
    "envelope": {18432: 82, 16000: 81, 8000: 80, 24000: 85, 513: None},
    "filter": {18432: 82, 16000: 84, 8000: 80, 24000: 80, 513: None},
    "pair": {18432: 80, 16000: 81, 8000: 80, 24000: 83, 513: None},
    "four": {18432: 81, 16000: 80, 8000: 81, 24000: 82, 513: None},
}
DEFAULT_SEED = 80


# ---- the batches ----------------------------------------------------------------------------------------------------------------
_FILLER = {}


def filler(bname):
    """The batch's packed audio and payloads with seeded noise in every slot, built once: one default_rng array, sliced."""
    if bname not in _FILLER:
        lengths = BATCHES[bname][0]
        rng = np.random.default_rng(20260 + len(lengths))
        audio = (0.1 * rng.standard_normal(sum(lengths))).astype(np.float32)
        wm = (2.0 * rng.integers(0, 2, (len(lengths), 20)) - 1.0).astype(np.float32)
        _FILLER[bname] = (audio, wm, np.concatenate([[0], np.cumsum(lengths)]))
    return _FILLER[bname]


def clip_seed(cname, n):
    s = SEEDS.get(cname, {}).get(n)
    return DEFAULT_SEED if s is None else s


def attack_seeds(bname):
    lengths = BATCHES[bname][0]
    seeds = [1000 + i for i in range(len(lengths))]
    for slot in COMPARED[bname]:
        seeds[slot] = ATTACK_SEED[lengths[slot]]
    return seeds


def big_session(rt, O, bname, cname, chain="named", **kw):
    """A begun session on the batch, its compared slots holding the clips chosen for chain `cname`; `chain` overrides the
    entries (None: no chain).  Asserts the run the batch was built to select and prints the partition."""
    lengths, run = BATCHES[bname]
    audio, wm, off = filler(bname)
    audio, wm = audio.copy(), wm.copy()
    for slot in COMPARED[bname]:
        a, bits = make_clip(clip_seed(cname, lengths[slot]), lengths[slot])
        audio[off[slot]: off[slot + 1]] = a
        wm[slot] = O.bits_to_bipolar(bits)
    batch = rt.Batch(lengths)
    pstride = (batch.scratch_bytes - 256) // (8 * batch.B)
    print(f"{bname}: {batch.B} clips, synth_run {batch.synth_run} (expected {run}), analysis_run {batch.analysis_run}, pstride {pstride}, "
          f"{batch.total_pooled} pooled rows")
    assert batch.synth_run == run == expected_synth_run(lengths)
    sess = rt.EmbedSession(plan_for(rt), det_for(rt, O), batch, **kw)
    seeds = attack_seeds(bname)
    if chain == "named":
        chain = CHAINS[cname]
    if chain is not None:
        sess.set_loop_attacks(chain, seeds)
    sess.begin(torch.from_numpy(audio).cuda(), torch.from_numpy(wm).cuda())
    return sess, batch, seeds


# ---- a. forward -----------------------------------------------------------------------------------------------------------------
def check_forward(rt, LA, cname, sess, batch, seeds, step, sample, tag):
    """Every chain by the check_forward of its kind's own module, with that module's bound, on the sampled clips."""
    chain = LA.parse_chain(CHAINS[cname])
    if cname in ("noise", "suppression", "envelope"):
        forward_01(LA, sess, batch, chain, seeds, step, tag, sample=sample)
    elif cname == "reverb":
        forward_reverb(rt, LA, sess, batch, chain, seeds, step, tag, sample=sample)
    elif cname == "filter":
        forward_filter(rt, LA, sess, batch, chain, seeds, step, tag, sample=sample)
    else:
        by = {"speed": forward_speed, "stretch": forward_stretch, "pair": forward_stretch, "pitch": forward_pitch, "four": forward_pitch,
              "pv": forward_pv, "crop": forward_delete, "anywhere": forward_delete}[cname]
        by(LA, sess, batch, chain, seeds, step, tag, sample=sample)


def forward_sample(bname, cname):
    """The compared slots.  The phase vocoder's restatement transforms the clip with torch.stft, which refuses the 512 samples of
    the 513-sample clip's signal (reflect padding of n_fft / 2 needs more): under that chain the clip is in the batch, and its
    buffer 12 is required to be finite, but there is no restatement to hold it against."""
    lengths = BATCHES[bname][0]
    return [s for s in COMPARED[bname] if not (cname == "pv" and lengths[s] == 513)]


FORWARD_CASES = [("R12", c) for c in CHAINS] + [(b, c) for b in ("R8", "R6", "U12") for c in SPLIT_AND_ENVELOPE]


@pytest.mark.parametrize("bname,cname", FORWARD_CASES, ids=[f"{b}-{c}" for b, c in FORWARD_CASES])
def test_forward_matches_the_restatement(rt, O, LA, bname, cname):
    """Buffer 12 of the compared clips against the restatement applied to the device's own N(N(buffer 9)), at step 0 and after
    iterate(3) (step 2), by the kind's existing check and bound."""
    sess, batch, seeds = big_session(rt, O, bname, cname, num_iterations=4)
    sample = forward_sample(bname, cname)
    sess.gradient()
    check_forward(rt, LA, cname, sess, batch, seeds, 0, sample, f"{bname} {cname}")
    sess.iterate(3)
    assert int(sess.step.cpu()[0]) == 3
    check_forward(rt, LA, cname, sess, batch, seeds, 2, sample, f"{bname} {cname}")
    z = sess.attacked[: sum(batch.out_lengths[:len(HEAD)])]
    assert bool(torch.isfinite(z).all()) and float(z.abs().max()) > 0.0


# ---- b. first gradient, loss and prediction ---------------------------------------------------------------------------------------
_ORACLE = {}


def oracle(O, LA, cname, n):
    """Gradient, loss, prediction and kink distance of the float64 and the float32 composition for the clip of this chain and
    length; it does not depend on the batch, so it is computed once for all of them."""
    if (cname, n) not in _ORACLE:
        clip, bits = make_clip(SEEDS[cname][n], n)
        wm = np.asarray(O.bits_to_bipolar(bits), dtype=np.float32)
        chain = LA.parse_chain(CHAINS[cname])
        _ORACLE[cname, n] = tuple(oracle_gradient(O, LA, chain, ATTACK_SEED[n], clip, wm, dt) for dt in (torch.float64, torch.float32))
    return _ORACLE[cname, n]


def alone_figures(rt, O, cname, bname, sess, batch, g, dsp_path):
    """Diagnostic, printed and not asserted: the head clips inside the batch against the same five clips alone (run 4)."""
    pairs = [make_clip(clip_seed(cname, n), n) for n in HEAD]
    small = rt.Batch(HEAD)
    one = rt.EmbedSession(plan_for(rt), det_for(rt, O), small, use_graph=False, dsp_path=dsp_path)
    one.set_loop_attacks(CHAINS[cname], [ATTACK_SEED[n] for n in HEAD])
    one.begin(small.pack([p[0] for p in pairs]), torch.from_numpy(np.stack([O.bits_to_bipolar(p[1]) for p in pairs]).astype(np.float32)).cuda())
    g1 = one.gradient()
    torch.cuda.synchronize()
    nf = small.total_frames
    assert small.synth_run == 4 and batch.frame_offsets[len(HEAD)] == nf
    dl = float((sess.loss[:5] - one.loss).abs().max())
    dp = float((sess.pred[:5] - one.pred).abs().max())
    dg = max(float((g[a:b] - g1[a:b]).norm() / g1[a:b].norm()) for a, b in zip(small.frame_offsets[:-1], small.frame_offsets[1:]))
    print(f"{bname} {cname} {dsp_path}: head clips in the batch against the same clips alone (run 4): loss {dl:.2e}, prediction {dp:.2e}, "
          f"gradient rel L2 {dg:.2e}")


GRADIENT_CASES = [("R12", c, d) for c in CHAINS for d in ("stream", "staged")] + \
                 [(b, c, "stream") for b in ("R8", "R6", "U12") for c in CHAINS]


@pytest.mark.parametrize("bname,cname,dsp_path", GRADIENT_CASES, ids=[f"{b}-{c}-{d}" for b, c, d in GRADIENT_CASES])
def test_first_gradient(rt, O, LA, bname, cname, dsp_path):
    """aware_embed_gradient, loss and prediction of the compared clips against autograd over the float64 restatement composed
    with the oracle's loop body, by the rule of loop_support.check_gradient: within four times the float32 composition's own
    distance from the float64 one, at least 2e-5 (gradient, relative L2) and 1e-6 (loss, prediction); no compared clip within
    KINK of a LeakyReLU kink in either precision."""
    lengths = BATCHES[bname][0]
    sess, batch, seeds = big_session(rt, O, bname, cname, use_graph=False, dsp_path=dsp_path)
    g = sess.gradient()
    torch.cuda.synchronize()
    if bname == "R12":
        alone_figures(rt, O, cname, bname, sess, batch, g, dsp_path)
    loss, pred = sess.loss.cpu().numpy(), sess.pred.cpu().numpy()
    checked = []
    for slot in COMPARED[bname]:
        n = lengths[slot]
        if SEEDS[cname].get(n) is None:
            assert n not in (18432, 16000)
            continue
        (ref, l, p, kink), (r32, l32, p32, kink32) = oracle(O, LA, cname, n)
        floor = float((r32 - ref).norm() / ref.norm())
        lfloor, pfloor = abs(l32 - l), float(np.abs(p32 - p).max())
        mine = g[batch.frame_offsets[slot]: batch.frame_offsets[slot + 1], :225].cpu().T.double()
        rel = float((mine - ref).norm() / ref.norm())
        lerr, perr = abs(loss[slot] - l), float(np.abs(pred[slot] - p).max())
        gb, lb, pb = max(4 * floor, 2e-5), max(4 * lfloor, 1e-6), max(4 * pfloor, 1e-6)
        print(f"{bname} {cname} {dsp_path} slot {slot} (n = {n}): loss err {lerr:.1e} (float32 restatement {lfloor:.1e}), pred err {perr:.1e} "
              f"({pfloor:.1e}), gradient rel L2 {rel:.2e} ({floor:.2e}), nearest LeakyReLU kink {kink:.1e} / {kink32:.1e}; "
              f"error / bound: loss {lerr / lb:.3f}, pred {perr / pb:.3f}, gradient {rel / gb:.3f}")
        assert min(kink, kink32) >= KINK, (slot, kink, kink32)
        assert lerr <= lb and perr <= pb, (slot, lerr, lfloor, perr, pfloor)
        assert rel <= gb, (slot, rel, floor)
        checked.append(n)
    assert {18432, 16000} & set(lengths) <= set(checked) and checked


# ---- c. prob 0 is the plain loop ----------------------------------------------------------------------------------------------------
_PLAIN = {}


def plain_loop(rt, O, bname):
    if bname not in _PLAIN:
        plain, _, _ = big_session(rt, O, bname, "plain", chain=None, num_iterations=21)
        plain.iterate(20)
        gp = plain.gradient()
        torch.cuda.synchronize()
        _PLAIN[bname] = tuple(t.clone() for t in (plain.coef, plain.best_coef, plain.loss, plain.best_loss, gp))
    return _PLAIN[bname]


@pytest.mark.parametrize("cname", SPLIT_AND_ENVELOPE)
@pytest.mark.parametrize("bname", ["R12", "R6"])
def test_prob_0_is_the_plain_loop(rt, O, bname, cname):
    """An entry that never fires against the loop without a chain, over the whole batch: coefficients, best coefficients and
    losses after 20 steps and the gradient of step 20, bit for bit.

    The envelope case exposed that a chain of element-wise kinds alone never took the plain loop's path: it normalises twice
    in front of the chain and twice behind it, the plain loop only twice, and N(N(.)) is not idempotent in f32, so
    [gain_envelope(prob 0)] differed from the plain loop in the last bit of the first forward pass at every run length (after
    20 steps: 9.2e-5 in the coefficients on [16000, 8000, 24000] at run 4, 7.2e-1 on R12, 1.2 on R6).  A chain that holds an
    envelope now takes the idle rule of the splitting chains (csrc/capi.hip chain_stage_launch)."""
    chain = [dict(a, prob=0.0) for a in CHAINS[cname]]
    att, batch, _ = big_session(rt, O, bname, "plain", chain=chain, num_iterations=21)
    att.iterate(20)
    ga = att.gradient()
    torch.cuda.synchronize()
    coef, best_coef, loss, best_loss, gp = plain_loop(rt, O, bname)
    print(f"{bname} {cname}, prob 0 against the plain loop after 20 steps: max |coef difference| = {float((coef - att.coef).abs().max()):.3e}, "
          f"loss difference {float((loss - att.loss).abs().max()):.3e}, gradient rel L2 {float((gp - ga).norm() / gp.norm()):.3e}")
    assert torch.equal(coef, att.coef) and torch.equal(best_coef, att.best_coef)
    assert torch.equal(loss, att.loss) and torch.equal(best_loss, att.best_loss)
    assert torch.equal(gp, ga)


# ---- d. graph replay ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", ["filter_noise", "pitch"])
def test_graph_replay_is_bit_identical_and_redraws(rt, O, cname):
    chain = {"filter_noise": [dict(BF, prob=0.75), NOISE10], "pitch": [dict(PITCH, prob=0.75)]}[cname]
    out = []
    for use_graph in (True, False):
        sess, batch, _ = big_session(rt, O, "R12", "plain", chain=chain, num_iterations=40, use_graph=use_graph)
        zs, losses = [], []
        sess.iterate(32)
        for _ in range(8):
            sess.iterate(1)
            zs.append(sess.attacked.clone())
            losses.append(sess.loss.clone())
        torch.cuda.synchronize()
        assert int(sess.step.cpu()[0]) == 40
        out.append((sess.coef.clone(), sess.best_coef.clone(), sess.best_loss.clone(), torch.stack(losses), torch.stack(zs)))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    head = sum(batch.out_lengths[:len(HEAD)])
    zs = out[0][4][:, :head].cpu()
    assert len({zs[i].numpy().tobytes() for i in range(8)}) == 8          # the draws are keyed by the device step counter


# ---- e. a mixture is its chains -----------------------------------------------------------------------------------------------------
def test_a_mixture_is_its_chains(rt, O, LA):
    """A mixture of [pitch shift, noise] and [envelope of 64 samples] on R12 at step 0 against, per head clip, a session on the
    same batch that holds only the chain the clip drew: buffers 12 and 9, loss, prediction and the rows of the gradient, bit
    for bit."""
    lengths, run = BATCHES["R12"]
    mixture = LA.parse_mixture([{"weight": 0.5, "chain": [PITCH, NOISE10]}, {"weight": 0.5, "chain": [ENV_SHORT]}])
    s0 = 0
    while set(LA.mixture_choices(list(range(s0, s0 + len(HEAD))), 0, weights(mixture)).tolist()) != {0, 1}:
        s0 += 1
    seeds = list(range(s0, s0 + len(lengths)))
    choice = LA.mixture_choices(seeds[:len(HEAD)], 0, weights(mixture))
    kw = dict(num_iterations=4)
    mix, batch = mixture_session(rt, O, lengths, seeds, mixture=mixture, **kw)
    assert batch.synth_run == run
    g = mix.gradient()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(mix.choices.cpu().numpy()[:len(HEAD)], choice)
    z, y, loss, pred = mix.attacked.clone(), mix._view(9, (batch.total_out,)).clone(), mix.loss.clone(), mix.pred.clone()
    for c in (0, 1):
        one, _ = mixture_session(rt, O, lengths, seeds, chain=mixture[c]["chain"], **kw)
        g1 = one.gradient()
        torch.cuda.synchronize()
        y1 = one._view(9, (batch.total_out,))
        for b in np.flatnonzero(choice == c):
            dz = (z[span(batch, b)] - one.attacked[span(batch, b)]).abs()
            print(f"clip {b} (n = {lengths[b]}) drew chain {c}: max |buffer 12 difference| = {float(dz.max()):.3e} over {int((dz > 0).sum())} samples")
            assert torch.equal(y[span(batch, b)], y1[span(batch, b)]), (b, c)
            assert torch.equal(z[span(batch, b)], one.attacked[span(batch, b)]), (b, c)
            assert torch.equal(loss[b], one.loss[b]) and torch.equal(pred[b], one.pred[b]), (b, c)
            gm, g1m = g[rows(batch, b)], g1[rows(batch, b)]
            print(f"    loss {float(loss[b]):.6f} / {float(one.loss[b]):.6f}, max |gradient| {float(gm.abs().max()):.3e} / {float(g1m.abs().max()):.3e}, "
                  f"rows that differ {int((gm != g1m).any(dim=1).sum())} of {gm.shape[0]}, not finite {int((~torch.isfinite(gm)).sum())}")
            assert torch.equal(gm, g1m), (b, c)
            # the 513-sample clip has three frames, one pooled row: the detector's instance norm over time maps it to a constant,
            # so its loss is 1 and its gradient exactly zero under every chain; every other clip's gradient is not
            assert (float(gm.abs().max()) > 0.0) == (lengths[b] != 513), (b, c)
