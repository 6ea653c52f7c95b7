"""The tiled excerpt inside the embed loop (EXTENSION, chain kind 10) on the device: the kernel of csrc/loop_excerpt_kernels.hip in
both directions, alone and inside the loop, against numpy and the torch restatement aware_amd/embedding/loop_attacks.py composed
with the oracle's loop body.  The forward pass copies and the adjoint adds in float32 over ascending periods, as the restatement
does, so the comparisons are bit for bit wherever no noise entry follows.

Shapes: clips [8000] * 2 (7936 output samples: an excerpt drawn longer than that is the identity), [16000] * 2 (15872, more than
one synthesis run per clip) and the ragged [16000, 8000]; [16000, 8000, 513] for the clip shorter than every excerpt; stand-alone
clips of 4099, 1025 and 2048 samples, packed back to back so that the second starts at an odd offset.

Run on the MI355X box:  python -m pytest tests/test_gpu_loop_excerpt.py -m gpu -q -s"""
import ctypes as C

import numpy as np
import pytest
import torch

from loop_support import CHAIN_BOUND, DS, EV, FB, KINK, LA, LONG, NO, NOISE10, O, PS, PV, RAGGED, RV, SHORT, SP, ST, SU, SUP, XC
from loop_support import attacked, bits_equal, check_gradient, device_x, does_not_fire_keeps_its_bits, ex_entries
from loop_support import forward_at_run_length, forward_at_steps_0_2_17, graph_replay_bits, mixture_is_its_chains, norm2
from loop_support import older_chains_workspace, plus_zero, prob_0_is_the_plain_loop, rt, sampled, session, stereo_round_trip
from loop_support import synthesis, value_claim_setup

pytestmark = pytest.mark.gpu

EX = {"kind": "excerpt", "seconds": [0.1875, 0.625]}
CHAINS = {"excerpt": [EX], "suppression_excerpt": [SUP, EX], "excerpt_noise": [EX, NOISE10]}
assert CHAIN_BOUND == 1.13e-6                              # the project's bound for the loop's attacked signal


def tile(x, start, L):
    return x[start + np.arange(len(x)) % L]


def tile_adjoint(g, start, L):
    """float32, ascending periods: the accumulator is the first period, every further one is one rounded addition."""
    n = len(g)
    acc = g[:L].copy()
    for lo in range(L, n, L):
        w = min(L, n - lo)
        acc[:w] = acc[:w] + g[lo:lo + w]
    out = np.zeros(n, dtype=np.float32)
    out[start:start + L] = acc
    return out


def terms(n, start, L, i):
    """How many terms the adjoint adds at position i."""
    return len(range(i - start, n, L)) if start <= i < start + L else 0


def drawn(LA, chain, seed, step, ny):
    """(fires, start, L) of the chain's excerpt for this clip at this step; L = ny where it does not fire."""
    chain = LA.parse_chain(chain)
    j = [a["kind"] for a in chain].index("excerpt")
    r = LA.entry_draw(seed, step, j)
    on = LA.fires(r[0], chain[j]["prob"])
    start, L = LA.excerpt_draw(chain[j], r, ny, 16000, on=on)
    return on, start, L


# ---- 1. the operator alone ----------------------------------------------------------------------------------------------------
def raw_tile(rt, x, starts, lengths, adjoint=False):
    """aware_excerpt_tile itself, without runtime.excerpt_tile's checks: the entry clamps what it is given."""
    from aware_amd.runtime import _ptr, _stream, check, load_library
    out = rt.Ragged(torch.full((sum(x.lengths),), float("nan"), dtype=torch.float32, device=x.data.device), x.lengths)
    sd = torch.tensor(starts, dtype=torch.int32, device=x.data.device)
    ld = torch.tensor(lengths, dtype=torch.int32, device=x.data.device)
    check(load_library().aware_excerpt_tile(_ptr(x.data), _ptr(x.d_off), _ptr(x.d_len), x.B, x.max_len, _ptr(sd), _ptr(ld), _ptr(out.data),
                                            int(adjoint), _stream()), "aware_excerpt_tile")
    return out


def test_excerpt_tile_is_numpy_bit_for_bit(rt):
    """aware_excerpt_tile, forward and adjoint, against numpy on uint32 views, three clips of 4099, 1025 and 2048 floats in one
    call, the second at float offset 4099: L = 1024, n - 1, n and above n (clamped by the entry); start 0, n - L and odd; a period
    that crosses a workgroup's chunk of 2048 samples; adjoint positions with exactly one, two and three terms; lengths below the
    kernel's stride of 256, which only this entry accepts."""
    rng = np.random.default_rng(23)
    lengths = [4099, 1025, 2048]
    xs = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    gs = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    x, g = rt.Ragged.from_list(xs), rt.Ragged.from_list(gs)
    assert list(x.offsets[:3]) == [0, 4099, 5124]
    cases = [([0, 0, 0], [1024, 1024, 1024]), ([4099 - 1024, 1, 1024], [1024, 1024, 1024]), ([333, 1, 77], [1500, 1024, 1025]),
             ([0, 0, 0], [4098, 1024, 2047]), ([1, 1, 1], [4098, 1024, 2047]), ([0, 0, 0], [4099, 1025, 2048]),
             ([2051, 0, 1001], [2047, 513, 1001]), ([7, 999, 0], [255, 26, 256]), ([4098, 0, 13], [1, 3, 300])]
    seen = set()
    for starts, ls in cases:
        z = rt.excerpt_tile(x, starts, ls).to_list()
        gx = rt.excerpt_tile(g, starts, ls, adjoint=True).to_list()
        for xi, gi, zi, gxi, s, L in zip(xs, gs, z, gx, starts, ls):
            n = len(xi)
            assert bits_equal(zi, tile(xi, s, L)), (starts, ls)
            assert bits_equal(gxi, tile_adjoint(gi, s, L)), (starts, ls)
            assert np.all(gxi[:s].view(np.uint32) == 0) and np.all(gxi[s + L:].view(np.uint32) == 0)      # +0.0 outside the excerpt
            if L == n:
                assert bits_equal(zi, xi) and bits_equal(gxi, gi)
            seen |= {terms(n, s, L, i) for i in (s, s + L - 1)}
    assert terms(4099, 333, 1500, 333) == 3 and terms(4099, 333, 1500, 333 + 1499) == 2 and terms(4099, 1, 4098, 4098) == 1
    assert {1, 2, 3} <= seen
    # the entry clamps: a length above n is n, below 1 is 1, and the start moves inside the clip
    for starts, ls, cs, cl in (([0, 0, 0], [4104, 1030, 1 << 30], [0, 0, 0], lengths), ([5, 5, -5], [4104, 1030, 2000], [0, 0, 0], [4099, 1025, 2000]),
                               ([4000, 1000, 2047], [1024, 1024, 0], [4099 - 1024, 1, 2047], [1024, 1024, 1])):
        z = raw_tile(rt, x, starts, ls).to_list()
        gx = raw_tile(rt, g, starts, ls, adjoint=True).to_list()
        for xi, gi, zi, gxi, s, L in zip(xs, gs, z, gx, cs, cl):
            assert bits_equal(zi, tile(xi, s, L)) and bits_equal(gxi, tile_adjoint(gi, s, L)), (starts, ls)
    # one value for all clips; a clip alone gives the same bits as inside a batch, wherever it starts
    both = rt.excerpt_tile(x, 1, 1024).to_list()
    for xi, zi in zip(xs, both):
        assert bits_equal(zi, tile(xi, 1, 1024))
        assert bits_equal(rt.excerpt_tile(rt.Ragged.from_list([xi]), [1], [1024]).to_list()[0], zi)
    for bad in (([0], [1024]), ([0, 0, 0], [4100, 1024, 1024]), ([-1, 0, 0], [1024] * 3), ([0, 2, 0], [1024] * 3), ([0, 0, 0], [1024, 0, 1024])):
        with pytest.raises(ValueError):
            rt.excerpt_tile(x, *bad)


# ---- 2. forward inside the loop -----------------------------------------------------------------------------------------------
def check_forward(LA, sess, batch, chain, seeds, step, tag, sample=None):
    torch.cuda.synchronize()
    kinds = [a["kind"] for a in chain]
    exact = kinds[-1] != "gaussian_noise"
    worst = 0.0
    for b, y, z in sampled(sess, batch, sample):
        on, start, L = drawn(LA, chain, seeds[b], step, len(y))
        assert on and 1 <= L <= len(y) and 0 <= start <= len(y) - L
        if exact:
            ref = LA.apply_chain(torch.from_numpy(device_x(y.numpy()))[None], chain, [seeds[b]], step)[0].numpy()
            if "sample_suppression" in kinds:                                              # the device's suppressed zeros are +0.0
                assert not np.any(np.signbit(z.numpy()) & (z.numpy() == 0))
                ref = plus_zero(ref)
            assert bits_equal(z.numpy(), ref), (tag, step, b, start, L)
        ref = LA.apply_chain(norm2(y.double())[None], chain, [seeds[b]], step)[0]
        worst = max(worst, float((z.double() - ref).abs().max() / ref.abs().max()))
    print(f"{tag}, step {step}: max |z - float64 restatement| / peak = {worst:.2e}" + (", bit-identical to the float32 one" if exact else ""))
    assert worst < CHAIN_BOUND, (tag, step, worst)


@pytest.mark.parametrize("name", list(CHAINS))
@pytest.mark.parametrize("lengths", [SHORT, LONG, RAGGED], ids=["short", "long", "ragged"])
def test_forward_matches_the_restatement(rt, O, LA, lengths, name):
    """Buffer 12 at steps 0, 2 and 17.  The excerpt alone and behind a suppression: bit-identical to the restatement on
    x = N(N(buffer 9)) in the device's rounding.  With noise behind it: within CHAIN_BOUND = 1.13e-6 of the peak of the float64
    restatement (all chains are held to that as well).  The draws differ from step to step."""
    chain = LA.parse_chain(CHAINS[name])
    batch, seeds = forward_at_steps_0_2_17(rt, O, LA, chain, lengths, name, check_forward)
    if batch.out_lengths[0] == 15872:                                                       # every excerpt is shorter than this clip
        assert len({drawn(LA, chain, seeds[0], s, 15872)[1:] for s in (0, 2, 17)}) == 3
        assert all(drawn(LA, chain, seeds[0], s, 15872)[2] < 15872 for s in (0, 2, 17))
    else:                                                                                   # 7936 samples: an excerpt drawn longer is the identity
        assert len({drawn(LA, chain, sd, s, 7936)[1:] for sd in seeds for s in (0, 2, 17)}) >= 3


def test_a_clip_shorter_than_the_excerpt_is_left_alone(rt, O, LA):
    """A batch with a 513-sample clip (512 output samples, below L_lo = 3000): the chain is accepted, that clip's buffer 12 is
    N(N(buffer 9)) in the device's rounding bit for bit at every step, and the other clips are tiled."""
    lengths, seeds = [16000, 8000, 513], [3, 4, 5]
    chain = LA.parse_chain([EX])
    sess, batch, _, _ = session(rt, O, lengths, [30, 31, 32], chain, seeds, num_iterations=20)
    assert batch.out_lengths == [15872, 7936, 512]
    sess.gradient()
    for step in (0, 2, 5):
        if step:
            sess.iterate(3)
        torch.cuda.synchronize()
        for b, (y, z) in enumerate(zip(synthesis(sess, batch), attacked(sess, batch))):
            on, start, L = drawn(LA, chain, seeds[b], step, len(y))
            x = device_x(y.numpy())
            assert bits_equal(z.numpy(), tile(x, start, L)), (step, b)
            if b == 2:
                assert L == 512 and start == 0 and bits_equal(z.numpy(), x)
        assert drawn(LA, chain, seeds[0], step, 15872)[2] < 15872


# ---- 3. first gradient ----------------------------------------------------------------------------------------------------------
# Clip seeds chosen on the CPU so that both the float64 and the float32 restatement keep every LeakyReLU argument of both clips
# at least KINK = 8e-6 from its kink (seeds 80 to 99 tried, each clip with its own attack seed: 5 for the first, 7 for the second).
# Ragged [16000, 8000], the entry alone: seeds 81 and 82, 1.8e-5 / 1.3e-4 (80 as the long clip was at 2.8e-6; 80 as the short one
# at 3.3e-6).  Two long clips between a suppression and noise: seeds 80 and 81, 4.4e-5 / 1.9e-5 (81 as the first was at 1.4e-6,
# 82 as the second at 4.0e-6).  The draws at step 0: alone (start, L) = (1368, 3691) and (2588, 3516); between, entry 1,
# (5547, 9022) and (2841, 6314): every position of the long clips' adjoint has two to five terms.
SEED0, SEED0_BETWEEN = 81, 80
assert KINK == 8e-6
# the module's pieces of loop_support.check_gradient, which states the rule and its bounds
GRADIENT = dict(drawn=drawn, describe=lambda d: f"start = {d[1]}, L = {d[2]}", exercised=lambda d, i, ny: d[0] and d[2] < ny)


@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
def test_first_gradient(rt, O, LA, dsp_path):
    check_gradient(rt, O, LA, [EX], RAGGED, SEED0, **GRADIENT, dsp_path=dsp_path)


def test_first_gradient_f32_dense(rt, O, LA):
    check_gradient(rt, O, LA, [EX], RAGGED, SEED0, **GRADIENT, conv_pipe="f32", mel="dense")


@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
def test_first_gradient_between_other_entries(rt, O, LA, dsp_path):
    """A suppression in front and noise behind: the stages on both sides."""
    check_gradient(rt, O, LA, [SUP, EX, NOISE10], LONG, SEED0_BETWEEN, **GRADIENT, dsp_path=dsp_path)


# ---- 4. per-clip and replay behaviour ---------------------------------------------------------------------------------------------
def test_a_clip_that_does_not_fire_keeps_its_bits(rt, O, LA):
    """prob 0.5 on three clips, 8 steps: where the entry does not fire, buffer 12 is N(N(buffer 9)) in the device's rounding,
    bit for bit; where it fires it is the tiling of that.  Both occur."""
    does_not_fire_keeps_its_bits(rt, O, LA, EX, drawn, apply=lambda x, z, d: bits_equal(z, tile(x, d[1], d[2])),
                                 fired=lambda d, ny: d[0] and d[2] < ny)


def test_prob_0_is_the_plain_loop(rt, O):
    """An excerpt that never fires against the loop without a chain: coefficients, best coefficients and losses after 20 steps
    and the gradient of step 20, bit for bit, alone and between two older entries that never fire either, on both dsp_paths."""
    prob_0_is_the_plain_loop(rt, O, ([dict(EX, prob=0.0)], [dict(SUP, prob=0.0), dict(EX, prob=0.0), dict(NOISE10, prob=0.0)]))


@pytest.mark.parametrize("lengths", [LONG, RAGGED], ids=["long", "ragged"])
def test_graph_replay_is_bit_identical_and_redraws(rt, O, LA, lengths):
    chain = LA.parse_chain([dict(EX, prob=0.75), NOISE10])
    _, batch = graph_replay_bits(rt, O, chain, lengths)
    # the draws are keyed by the device step counter: both start and L of clip 0 (seed 0) move from step to step
    n0 = batch.out_lengths[0]
    draws = [drawn(LA, chain, 0, s, n0) for s in range(32, 40)]
    fired = [d for d in draws if d[0]]
    assert len({d[1] for d in fired}) >= 4 and len({d[2] for d in fired}) >= 4, draws
    # a second chain without the noise: the replayed graph's buffer 12 is periodic with the step's own L at every step
    bare = LA.parse_chain([EX])
    sess, batch, _, _ = session(rt, O, lengths, list(range(50, 50 + len(lengths))), bare, num_iterations=40, use_graph=True)
    sess.iterate(4)
    seen = set()
    for step in range(4, 10):
        sess.iterate(1)
        torch.cuda.synchronize()
        z = attacked(sess, batch)[0].numpy()
        _, start, L = drawn(LA, bare, 0, step, n0)
        assert L < n0 and np.array_equal(z[L:], z[:n0 - L]) and not np.array_equal(z[L + 1:], z[:n0 - L - 1]), (step, L)
        seen.add((start, L))
    assert len(seen) == 6


def test_a_mixture_is_its_chains(rt, O, LA):
    """A mixture of {excerpt, noise} and {reverberation} at step 0: buffer 14 holds the host's choices, and every clip's buffer 12
    (with buffer 9, loss, prediction and its rows of the coefficient gradient) is bit for bit that of a session that holds only the
    chain the clip drew; the clips of the excerpt chain are within CHAIN_BOUND of the float64 restatement."""
    mixture_is_its_chains(rt, O, LA, [EX, NOISE10], [{"kind": "reverberation", "rt60": [0.1, 0.3]}], bound=CHAIN_BOUND)


@pytest.mark.parametrize("bname", ["R12", "R8", "R6"])
def test_forward_at_every_synthesis_run_length(rt, O, LA, bname):
    """The batches of tests/test_loop_run_rule_host.py that select synthesis runs of 12, 8 and 6 hop blocks: buffer 12 of the five
    head clips (18432, 16000, 8000, 24000 and 513 samples) at steps 0 and 2, bit for bit the restatement on N(N(buffer 9)) in the
    device's rounding.  A workgroup's share of a clip then spans up to 3072 samples, which holds a whole period of the shortest
    excerpt and a wrap."""
    forward_at_run_length(rt, O, LA, bname, "excerpt", LA.parse_chain([EX]), check_forward)


# ---- 5. workspace and error codes -------------------------------------------------------------------------------------------------
def test_workspace_bytes(rt, O):
    """The seven older chains need what they needed; a chain with the kind needs what the same chain with a deletion in its place
    needs; a refused chain is sized by the older kind, as before."""
    size, nb, _ = older_chains_workspace(rt, O)
    for with_xc, with_ds in (([XC], [DS]), ([NO, XC], [NO, DS]), ([NO, SU, XC, NO], [NO, SU, DS, NO]), ([EV, XC, EV], [EV, DS, EV])):
        assert size(with_xc) == size(with_ds) > nb["noise"]
    for other in (RV, SP, ST, PS, PV, DS, FB):
        assert size([XC, other]) == size([other, XC]) == size([other])


def test_entry_point_error_codes(rt, O):
    from aware_amd._lib import LoopAttack
    sess, batch, _, _ = session(rt, O, RAGGED, [64, 65], None, num_iterations=20, use_graph=False)
    lib = sess.lib
    nb = lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries([XC]), 1)
    big = max(nb, lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries([RV]), 1),
              lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries([PV]), 1)) + 8 * batch.total_out + 512
    ws = torch.empty(big, dtype=torch.uint8, device="cuda")
    seeds = (C.c_uint32 * 2)(1, 2)
    assert batch.out_lengths == [15872, 7936]

    def call(entries, n=None, wsb=big, sd=seeds):
        return lib.aware_embed_set_loop_attacks_ex(sess.h, ex_entries(entries), len(entries) if n is None else n, sd,
                                                   C.c_void_p(ws.data_ptr()), wsb, None)

    old = (LoopAttack * 1)(LoopAttack(10, 3000.0, 1.0))
    assert lib.aware_embed_set_loop_attacks(sess.h, old, 1, seeds, C.c_void_p(ws.data_ptr()), big, None) == -1     # the older call
    nan, inf = float("nan"), float("inf")
    for p in ([1023.0, 10000.0, 0.0, 0.0], [0.0, 10000.0, 0.0, 0.0], [-3000.0, 10000.0, 0.0, 0.0], [3000.5, 10000.0, 0.0, 0.0],
              [3000.0, 10000.5, 0.0, 0.0], [10000.0, 3000.0, 0.0, 0.0], [3000.0, 2147483648.0, 0.0, 0.0], [3000.0, 10000.0, 1.0, 0.0],
              [3000.0, 10000.0, 0.0, 1.0], [3000.0, 10000.0, -1.0, 0.0], [nan, 10000.0, 0.0, 0.0], [3000.0, nan, 0.0, 0.0],
              [3000.0, inf, 0.0, 0.0], [3000.0, 10000.0, nan, 0.0], [3000.0, 10000.0, 0.0, nan], FB[2], [0.0]):
        assert call([(10, 1.0, p)]) == -1, p
    assert call([(10, 1.5, XC[2])]) == -1 and call([(11, 1.0, XC[2])]) == -1
    assert call([XC, XC]) == -1 and call([XC, NO, XC]) == -1                                                        # a second entry
    for other in (RV, SP, ST, PS, PV, DS, FB):                                                                      # forbidden neighbours
        assert call([XC, other]) == -1 and call([other, XC]) == -1, other
        assert call([other, NO, XC]) == -1 and call([XC, EV, other]) == -1, other
    assert call([ST, SP, XC]) == -1 and call([XC], n=5) == -1 and call([XC], sd=None) == -1
    assert call([XC], wsb=nb - 256) == -4 and call([NO, XC], wsb=nb - 256) == -4                                    # too small
    # an excerpt longer than a clip is no reason to refuse: the 7936-sample clip is below L_hi, and below this L_lo
    assert call([(10, 1.0, [8000.0, 10000.0, 0.0, 0.0])], wsb=nb) == 0 and call([(10, 1.0, [100000.0, 200000.0, 0.0, 0.0])], wsb=nb) == 0
    assert call([XC], wsb=nb) == 0 and lib.aware_embed_buffer(sess.h, 12) and not lib.aware_embed_buffer(sess.h, 13)
    assert call([], n=0) == 0 and not lib.aware_embed_buffer(sess.h, 12)
    assert call([NO, SU, XC, NO], wsb=nb) == 0 and call([EV, XC, EV, NO], wsb=nb) == 0
    assert call([(10, 0.0, [1024.0, 1024.0, 0.0, 0.0])], wsb=nb) == 0
    assert call([ST, SP]) == 0 and call([SP]) == 0 and call([RV]) == 0 and call([PS]) == 0 and call([PV]) == 0 and call([DS]) == 0
    assert call([FB]) == 0 and call([XC], wsb=nb) == 0
    sess.iterate(1)
    torch.cuda.synchronize()
    assert call([XC]) == -1 and call([], n=0) == -1                        # after the first iterate
    with pytest.raises(ValueError):
        sess.set_loop_attacks([EX], [1, 2])
    # the stand-alone entry, with real buffers: refused before anything is launched
    x = rt.Ragged.from_list([np.ones(2048, dtype=np.float32)])
    out, one = torch.empty(2048, device="cuda"), torch.tensor([1024], dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    args = lambda **kw: [kw.get("inp", p(x.data)), p(x.d_off), p(x.d_len), kw.get("B", 1), kw.get("max_len", 2048), p(one), p(one),
                         kw.get("out", p(out)), kw.get("adjoint", 0), None]
    assert lib.aware_excerpt_tile(*args()) == 0
    for kw in (dict(B=0), dict(B=65536), dict(max_len=0), dict(max_len=(1 << 30) + 1), dict(adjoint=2), dict(adjoint=-1), dict(out=p(x.data)),
               dict(out=None), dict(inp=None)):
        assert lib.aware_excerpt_tile(*args(**kw)) == -1, kw
    torch.cuda.synchronize()


# ---- 6. card round trip -----------------------------------------------------------------------------------------------------------
def test_stereo_service_round_trip_with_the_card_key(rt, tmp_path):
    """load() of a card with the excerpt in loop_attacks, then embed_watermark / detect_watermark on a stereo clip: every
    channel carries the payload."""
    stereo_round_trip(tmp_path, "[{kind: excerpt, seconds: [0.1875, 0.625], prob: 0.75}]", dict(EX, prob=0.75))


# ---- 7. the value claim on the device ---------------------------------------------------------------------------------------------
def test_value_claim_on_the_device(rt, O, tmp_path):
    """The host test's two embeddings (four 1 s clips, seeds 0..3, 400 steps) through AWAREEmbedder(loop_attacks=...) from an
    edited card, sliced on the host at the host test's points with its bounds: clean 0 % both, the plain mean over the slices of
    8000 and 6000 samples at least 10 %, the aware mean at most half of it.  Figures: DESIGN.md section 32."""
    from aware_amd.attacks import Excerpt
    from test_loop_excerpt_host import AWARE_CHAIN, STARTS
    from test_loop_gain_host import snr_db
    clips, bits, embed, ber = value_claim_setup(O, tmp_path)

    def table(det, y):
        n = y.shape[-1]
        return {L: [ber(det, y[:, s:s + L]) for s in STARTS if s + L <= n] for L in (12000, 8000, 6000, 4000, 3000)}

    y0, det = embed(None)
    y1, _ = embed(AWARE_CHAIN)
    y0, y1 = np.stack(y0), np.stack(y1)
    clean0, clean1 = ber(det, y0), ber(det, y1)
    t0, t1 = table(det, y0), table(det, y1)
    for L in t0:
        print(f"slices of {L:5d} samples: plain {np.mean(t0[L]):6.2f} %   excerpt-aware {np.mean(t1[L]):6.2f} %")
    m0, m1 = float(np.mean(t0[8000] + t0[6000])), float(np.mean(t1[8000] + t1[6000]))
    audio = np.stack(clips)
    print(f"clean BER plain {clean0:.2f} % / excerpt-aware {clean1:.2f} %; mean over the slices of 8000 and 6000: plain {m0:.2f} % / "
          f"aware {m1:.2f} %; SNR against the host: plain {snr_db(audio, y0):.1f} dB / aware {snr_db(audio, y1):.1f} dB")
    # the Excerpt attack is the slice
    cut = Excerpt(0.5, 0.25).apply_batch(rt.Ragged.from_list(list(y1)), 16000).to_list()
    assert all(np.array_equal(np.asarray(c), v[4000:12000]) for c, v in zip(cut, y1))
    assert clean0 == 0.0 and clean1 == 0.0
    assert m0 >= 10.0
    assert m1 <= 0.5 * m0
