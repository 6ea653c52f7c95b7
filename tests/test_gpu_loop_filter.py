"""Band filters inside the embed loop (EXTENSION, chain kind 9) on the device: the FIR kernel of csrc/loop_filter_kernels.hip alone
and inside the loop, against the float64 definition and the torch restatement aware_amd/embedding/loop_attacks.py composed with
the oracle's loop body.

Bounds.  Taps: at most 1 in magnitude, a handful of f32 roundings and a sine whose argument lies inside one turn: 1e-6 absolute.
Output: 255 f32 multiply-adds, worst case 256 * 2^-24 = 2^-16 relative to sum|h| * max|x|, against the float64 convolution with
the device's own taps.  Adjoint: the two sides differ by at most that per output, so 2^-15 * sum|h| * max|x| * sum|w|.

Shapes: stand-alone clips of [1, 100, 254, 255, 2047, 2048, 2049, 5000] samples and the workgroup's 4096-sample tile +- 1, packed
back to back so that every clip but the first starts where its neighbour ends; in the loop [8000] * 2, [16000] * 2 (more than
one synthesis run per clip) and [16000, 8000, 513] (the shortest clip the loop takes).

Run on the MI355X box:  python -m pytest tests/test_gpu_loop_filter.py -m gpu -q -s"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from loop_support import CHAIN_BOUND, DS, EV, FB, KINK, LA, LONG, NO, NOISE10, O, PS, PV, RAGGED, RV, SHORT, SP, ST, SU
from loop_support import bits_equal, check_gradient, device_x, does_not_fire_keeps_its_bits, ex_entries, forward_at_steps_0_2_17
from loop_support import graph_replay_bits, mixture_is_its_chains, norm2, older_chains_workspace, prob_0_is_the_plain_loop, rt
from loop_support import sampled, session, stereo_round_trip, value_claim_setup

pytestmark = pytest.mark.gpu

TINY = [16000, 8000, 513]
ALL4 = ["lowpass", "highpass", "bandpass", "bandstop"]
BF = {"kind": "band_filter", "response": ALL4, "freq": [600.0, 3800.0], "min_width": 400.0}
SUP = {"kind": "sample_suppression", "seconds": 0.02}      # this module's own: short enough for the 513-sample clip of TINY
CHAINS = {"filter": [BF], "suppression_filter": [SUP, BF], "noise_filter": [NOISE10, BF], "filter_noise": [BF, NOISE10]}
W = 1638
TILE = 4096                                                 # outputs per workgroup of the stand-alone grid (kFbTile)
assert CHAIN_BOUND == 1.13e-6


_TAPS = {}


def device_taps(rt, rs, c1, c2):
    """The device's own 255 taps of this filter, float64 copies (through the stand-alone entry on a one-sample clip)."""
    key = (int(rs), int(c1), int(c2))
    if key not in _TAPS:
        _, taps = rt.band_filter(rt.Ragged.from_list([np.ones(1, dtype=np.float32)]), [key[0]], [key[1]], [key[2]], return_taps=True)
        _TAPS[key] = taps[0, :255].cpu().numpy().astype(np.float64)
    return _TAPS[key]


@contextlib.contextmanager
def with_device_taps(rt, LA):
    """The restatement with the device's taps in place of the float64 ones: what the output bound is stated against."""
    keep = LA.filter_taps
    LA.filter_taps = lambda rs, c1, c2, dtype=np.float64: device_taps(rt, rs, c1, c2).astype(dtype)
    try:
        yield
    finally:
        LA.filter_taps = keep


def drawn(LA, chain, seed, step):
    """(fires, response, c1, c2) of the chain's band filter for this clip at this step."""
    chain = LA.parse_chain(chain)
    j = [a["kind"] for a in chain].index("band_filter")
    r = LA.entry_draw(seed, step, j)
    return (LA.fires(r[0], chain[j]["prob"]),) + LA.filter_draw(chain[j], r, 16000)


# ---- 1. the operator alone ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def alone(rt):
    rng = np.random.default_rng(23)
    lengths = [1, 100, 254, 255, 2047, 2048, 2049, 5000, TILE - 1, TILE, TILE + 1]
    xs = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    for x in xs:                                             # non-zero up to both ends: a halo that reads a neighbour shows
        x[0], x[-1] = 1.5, -1.5
    ws = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    return lengths, xs, ws, rt.Ragged.from_list(xs), rt.Ragged.from_list(ws)


# every response on every clip, edges at the limits (1 and 32767) and mid-band
FILTERS = [(1, 1, 1), (2, 32767, 32767), (4, 1, 32767), (8, 2458, 2458 + W), (1, 4096, 4096), (2, 14336, 14336),
           (4, 10240, 14336), (8, 32767 - W, 32767), (4, 16384, 16384 + W), (1, 32767, 32767), (2, 1, 1), (8, 1, 32767)]


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_taps_output_and_adjoint(rt, LA, alone, shift):
    lengths, xs, ws, x, w = alone
    pick = [FILTERS[(3 * b + shift * 5 + b // 4) % len(FILTERS)] for b in range(len(lengths))]
    rs, c1, c2 = ([p[i] for p in pick] for i in range(3))
    z, taps = rt.band_filter(x, rs, c1, c2, return_taps=True)
    aw = rt.band_filter(w, rs, c1, c2)
    torch.cuda.synchronize()
    taps = taps.cpu().numpy()
    worst_t = worst_z = worst_a = 0.0
    for b, (xb, wb, zb, awb) in enumerate(zip(xs, ws, z.to_list(), aw.to_list())):
        want = LA.filter_taps(rs[b], c1[b], c2[b])
        h = taps[b, :255].astype(np.float64)
        assert taps[b, 255] == 0.0
        terr = float(np.abs(h - want).max())
        worst_t = max(worst_t, terr)
        assert terr <= 1e-6, (b, pick[b], terr)
        ref = np.convolve(xb.astype(np.float64), h)[127:127 + len(xb)]
        bound = 2.0 ** -16 * np.abs(h).sum() * float(np.abs(xb).max())
        zerr = float(np.abs(zb.astype(np.float64) - ref).max())
        worst_z = max(worst_z, zerr / bound)
        assert zerr <= bound, (b, lengths[b], pick[b], zerr, bound)
        lhs, rhs = float(np.dot(zb.astype(np.float64), wb.astype(np.float64))), float(np.dot(xb.astype(np.float64), awb.astype(np.float64)))
        abound = 2.0 ** -15 * np.abs(h).sum() * float(np.abs(xb).max()) * float(np.abs(wb).sum())
        worst_a = max(worst_a, abs(lhs - rhs) / abound)
        assert abs(lhs - rhs) <= abound, (b, pick[b], lhs, rhs, abound)
    print(f"shift {shift}: max |taps - float64 definition| = {worst_t:.2e}; output error / bound = {worst_z:.3f}; adjoint gap / bound = {worst_a:.4f}")


def test_alone_details(rt, alone):
    lengths, xs, ws, x, w = alone
    # one value for all clips; a clip alone gives the same bits as inside a batch, wherever it starts
    both = rt.band_filter(x, 4, 4096, 9011).to_list()
    for b in (1, 4, 7):
        assert bits_equal(rt.band_filter(rt.Ragged.from_list([xs[b]]), [4], [4096], [9011]).to_list()[0], both[b])
    for bad in (([1], [1], [1]), (3, 4096, 4096), (1, -1, 4096), (1, 32768, 32768), (4, 9000, 4096), (0, 4096, 4096)):
        with pytest.raises(ValueError):
            rt.band_filter(x, *bad)
    from aware_amd import attacks as A
    got = A.BandFilter("bandpass", 1000.0, 2200.0).apply_batch(x, 16000).to_list()
    assert bits_equal(got[7], both[7]) and A.BandFilter("lowpass", 800.0).apply(xs[7], 16000).shape == (5000,)


@pytest.mark.parametrize("n", [1, 7, 9, 255, TILE + 1, TILE + 7, 2 * TILE + 9])
def test_nothing_is_written_past_the_clip(rt, n):
    """One clip whose last tile holds fewer samples than a thread produces, written into the middle of a buffer of sentinels:
    the sentinels on both sides keep their bits, and the clip is the filter's output."""
    rng = np.random.default_rng(n)
    xb = rng.standard_normal(n).astype(np.float32)
    big = torch.full((n + 64,), 7.25, dtype=torch.float32, device="cuda")
    out = rt.Ragged(big[32:32 + n], [n])
    z, taps = rt.band_filter(rt.Ragged.from_list([xb]), [8], [2458], [4096], return_taps=True, out=out)
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    assert np.all(got[:32] == 7.25) and np.all(got[32 + n:] == 7.25), n
    h = taps[0, :255].cpu().numpy().astype(np.float64)
    ref = np.convolve(xb.astype(np.float64), h)[127:127 + n]
    assert float(np.abs(got[32:32 + n] - ref).max()) <= 2.0 ** -16 * np.abs(h).sum() * float(np.abs(xb).max())
    with pytest.raises(ValueError):
        rt.band_filter(rt.Ragged.from_list([xb]), [8], [2458], [4096], out=rt.Ragged(big[:n + 1], [n + 1]))


# ---- 2. forward inside the loop -----------------------------------------------------------------------------------------------
def check_forward(rt, LA, sess, batch, chain, seeds, step, tag, sample=None):
    """Filter alone or behind a suppression: against the restatement with the device's taps on x = N(N(buffer 9)) in the device's
    rounding, to the stand-alone bound 2^-16 sum|h| max|x|.  With a noise entry the device's noise is f32 and within the project's
    CHAIN_BOUND of the peak of the float64 one: in front of the filter that passes through it, at most sum|h| times as large;
    behind it, it adds to the filter's own bound."""
    torch.cuda.synchronize()
    noisy = any(a["kind"] == "gaussian_noise" for a in chain)
    worst = 0.0
    for b, y, z in sampled(sess, batch, sample):
        on, rs, c1, c2 = drawn(LA, chain, seeds[b], step)
        assert on
        h = device_taps(rt, rs, c1, c2)
        x = torch.from_numpy(device_x(y.numpy())).double() if not noisy else norm2(y.double())
        with with_device_taps(rt, LA):
            ref = LA.apply_chain(x[None], chain, [seeds[b]], step)[0]
            j = [a["kind"] for a in chain].index("band_filter")
            xin = LA.apply_chain(x[None], chain[:j], [seeds[b]], step)[0] if j else x
        bound = 2.0 ** -16 * np.abs(h).sum() * float(xin.abs().max())
        if noisy:
            bound += CHAIN_BOUND * (np.abs(h).sum() * float(xin.abs().max()) + float(ref.abs().max()))
        err = float((z.double() - ref).abs().max())
        worst = max(worst, err / bound)
        assert err <= bound, (tag, step, b, (rs, c1, c2), err, bound)
    print(f"{tag}, step {step}: max |z - restatement| / bound = {worst:.3f}")


@pytest.mark.parametrize("name", list(CHAINS))
@pytest.mark.parametrize("lengths", [SHORT, LONG, TINY], ids=["short", "long", "tiny"])
def test_forward_matches_the_restatement(rt, O, LA, lengths, name):
    chain = LA.parse_chain(CHAINS[name])
    batch, seeds = forward_at_steps_0_2_17(rt, O, LA, chain, lengths, name, lambda *a: check_forward(rt, *a), shortest=(512, 7936, 15872))
    assert len({drawn(LA, chain, seeds[0], s)[1:] for s in (0, 2, 17)}) == 3


# ---- 3. first gradient ----------------------------------------------------------------------------------------------------------
# Clip seeds chosen on the CPU so that both the float64 and the float32 restatement keep every LeakyReLU argument of every clip at
# least KINK = 8e-6 from its kink (seeds 80 to 91 tried).  Ragged [16000, 8000], the entry alone: seeds 86 and 87, 2.4e-5 / 1.3e-5
# (80 as the long clip was at 1.2e-6, 82 at 4.1e-6).  Two long clips between a suppression and noise: seeds 89 and 90, 3.1e-5 /
# 5.6e-5 (87 as the first was at 2.2e-6, 85 as the second at 1.3e-7).
SEED0, SEED0_BETWEEN = 86, 89
assert KINK == 8e-6
# the module's pieces of loop_support.check_gradient, which states the rule and its bounds
GRADIENT = dict(drawn=lambda LA, chain, seed, step, ny: drawn(LA, chain, seed, step), exercised=lambda d, i, ny: d[0],
                describe=lambda d: f"response {d[1]}, c1 = {d[2]}, c2 = {d[3]}")


@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
def test_first_gradient(rt, O, LA, dsp_path):
    check_gradient(rt, O, LA, [BF], RAGGED, SEED0, **GRADIENT, dsp_path=dsp_path)


@pytest.mark.parametrize("dsp_path", ["stream", "staged"])
def test_first_gradient_between_other_entries(rt, O, LA, dsp_path):
    """A suppression in front and noise behind: the stages on both sides."""
    check_gradient(rt, O, LA, [SUP, BF, NOISE10], LONG, SEED0_BETWEEN, **GRADIENT, dsp_path=dsp_path)


# ---- 4. per-clip and replay behaviour ---------------------------------------------------------------------------------------------
def test_a_clip_that_does_not_fire_keeps_its_bits(rt, O, LA):
    """prob 0.5 on three clips, 8 steps: where the entry does not fire, buffer 12 is N(N(buffer 9)) in the device's rounding, bit
    for bit; where it fires it is the drawn filter of that, to the stand-alone bound.  Both occur."""
    def filtered(x, z, d):
        h = device_taps(rt, *d[1:])
        ref = np.convolve(x.astype(np.float64), h)[127:127 + len(x)]
        return float(np.abs(z - ref).max()) <= 2.0 ** -16 * np.abs(h).sum() * float(np.abs(x).max())

    does_not_fire_keeps_its_bits(rt, O, LA, BF, GRADIENT["drawn"], apply=filtered, fired=lambda d, ny: d[0])


def test_prob_0_is_the_plain_loop(rt, O):
    """A filter that never fires against the loop without a chain: coefficients, best coefficients and losses after 20 steps and
    the gradient of step 20, bit for bit, alone and between two older entries that never fire either, on both dsp_paths."""
    prob_0_is_the_plain_loop(rt, O, ([dict(BF, prob=0.0)], [dict(SUP, prob=0.0), dict(BF, prob=0.0), dict(NOISE10, prob=0.0)]))


@pytest.mark.parametrize("lengths", [LONG, RAGGED], ids=["long", "ragged"])
def test_graph_replay_is_bit_identical_and_redraws(rt, O, LA, lengths):
    chain = LA.parse_chain([dict(BF, prob=0.75), NOISE10])
    out, _ = graph_replay_bits(rt, O, chain, lengths)
    # the draws are keyed by the device step counter: the replayed graph's buffer 12 moves with them
    zs = out[4]
    assert len({zs[i].numpy().tobytes() for i in range(8)}) == 8
    draws = [drawn(LA, chain, 0, s) for s in range(32, 40)]
    assert len({d[1:] for d in draws if d[0]}) >= 4, draws


def test_a_mixture_is_its_chains(rt, O, LA):
    """A mixture of a filter chain and a noise chain at step 0 against, per clip, a session that holds only the chain the clip
    drew: buffers 12 and 9, loss, prediction and the rows of the coefficient gradient, bit for bit."""
    mixture_is_its_chains(rt, O, LA, [BF, NOISE10], [NOISE10])


# ---- 5. workspace and error codes -------------------------------------------------------------------------------------------------
def test_workspace_bytes(rt, O):
    """The seven older chains need what they needed; a chain with the kind needs what the same chain with a deletion in its place
    needs."""
    size, nb, _ = older_chains_workspace(rt, O)
    for with_fb, with_ds in (([FB], [DS]), ([NO, FB], [NO, DS]), ([NO, SU, FB, NO], [NO, SU, DS, NO]), ([EV, FB, EV], [EV, DS, EV])):
        assert size(with_fb) == size(with_ds) > nb["noise"]
    for other in (RV, SP, ST, PS, PV, DS):                  # a refused chain is sized by the older kind, as before
        assert size([FB, other]) == size([other, FB]) == size([other])


def test_entry_point_error_codes(rt, O):
    from aware_amd._lib import LoopAttack
    sess, batch, _, _ = session(rt, O, RAGGED, [64, 65], None, num_iterations=20, use_graph=False)
    lib = sess.lib
    nb = lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries([FB]), 1)
    big = max(nb, lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries([RV]), 1),
              lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries([PV]), 1)) + 8 * batch.total_out + 512
    ws = torch.empty(big, dtype=torch.uint8, device="cuda")
    seeds = (C.c_uint32 * 2)(1, 2)

    def call(entries, n=None, wsb=big, sd=seeds):
        return lib.aware_embed_set_loop_attacks_ex(sess.h, ex_entries(entries), len(entries) if n is None else n, sd,
                                                   C.c_void_p(ws.data_ptr()), wsb, None)

    old = (LoopAttack * 1)(LoopAttack(9, 15.0, 1.0))
    assert lib.aware_embed_set_loop_attacks(sess.h, old, 1, seeds, C.c_void_p(ws.data_ptr()), big, None) == -1     # the older call
    nan = float("nan")
    for p in ([0.0, 2458.0, 15565.0, 1638.0], [16.0, 2458.0, 15565.0, 1638.0], [1.5, 2458.0, 15565.0, 1638.0], [15.0, 0.0, 15565.0, 1638.0],
              [15.0, 2458.5, 15565.0, 1638.0], [15.0, 15565.0, 2458.0, 1638.0], [15.0, 2458.0, 15565.0, 0.0], [15.0, 2458.0, 15565.0, 1638.5],
              [15.0, 2458.0, 31130.0, 1638.0], [nan, 2458.0, 15565.0, 1638.0], [15.0, nan, 15565.0, 1638.0], [15.0, 2458.0, nan, 1638.0],
              [15.0, 2458.0, 15565.0, nan], [800.0, 8000.0, 0.0, 0.0], [0.0]):
        assert call([(9, 1.0, p)]) == -1, p
    assert call([(9, 1.5, FB[2])]) == -1 and call([(10, 1.0, FB[2])]) == -1
    assert call([FB, FB]) == -1 and call([FB, NO, FB]) == -1                                                        # a second entry
    for other in (RV, SP, ST, PS, PV, DS):                                                                          # forbidden neighbours
        assert call([FB, other]) == -1 and call([other, FB]) == -1, other
        assert call([other, NO, FB]) == -1 and call([FB, EV, other]) == -1, other
    assert call([ST, SP, FB]) == -1 and call([FB], n=5) == -1 and call([FB], sd=None) == -1
    assert call([FB], wsb=nb - 256) == -4 and call([NO, FB], wsb=nb - 256) == -4                                    # too small
    assert call([FB], wsb=nb) == 0 and lib.aware_embed_buffer(sess.h, 12) and not lib.aware_embed_buffer(sess.h, 13)
    assert call([], n=0) == 0 and not lib.aware_embed_buffer(sess.h, 12)
    assert call([NO, SU, FB, NO], wsb=nb) == 0 and call([EV, FB, EV, NO], wsb=nb) == 0
    assert call([(9, 0.0, [1.0, 1.0, 32766.0, 1.0])], wsb=nb) == 0
    assert call([ST, SP]) == 0 and call([SP]) == 0 and call([RV]) == 0 and call([PS]) == 0 and call([PV]) == 0 and call([DS]) == 0
    assert call([FB], wsb=nb) == 0
    sess.iterate(1)
    torch.cuda.synchronize()
    assert call([FB]) == -1 and call([], n=0) == -1                        # after the first iterate
    with pytest.raises(ValueError):
        sess.set_loop_attacks([BF], [1, 2])


# ---- 6. card round trip -----------------------------------------------------------------------------------------------------------
def test_stereo_service_round_trip_with_the_card_key(rt, tmp_path):
    """load() of a card with the filter in loop_attacks, then embed_watermark / detect_watermark on a stereo clip: every channel
    carries the payload."""
    stereo_round_trip(tmp_path, "[{kind: band_filter, response: [lowpass, highpass, bandpass, bandstop], freq: [600.0, 3800.0], "
                                "min_width: 400.0, prob: 0.75}]", dict(BF, prob=0.75))


# ---- 7. the value claim on the device ---------------------------------------------------------------------------------------------
def test_value_claim_on_the_device(rt, O, tmp_path):
    """The host test's two embeddings (four 1 s clips, seeds 0..3, 400 steps) through AWAREEmbedder(loop_attacks=...) from an
    edited card, under the host test's six Butterworth channels with its bounds: clean 0 % both, the plain mean over the six at
    least 10 %, the aware mean at most half of it.  Figures: DESIGN.md section 25."""
    from test_loop_filter_host import AWARE_CHAIN, butterworth_attacks
    from test_loop_gain_host import snr_db
    clips, bits, embed, ber = value_claim_setup(O, tmp_path)

    y0, det = embed(None)
    y1, _ = embed(AWARE_CHAIN)
    y0, y1 = np.stack(y0), np.stack(y1)
    clean0, clean1 = ber(det, y0), ber(det, y1)
    a0, a1 = butterworth_attacks(y0), butterworth_attacks(y1)
    b0 = {k: ber(det, v) for k, v in a0.items()}
    b1 = {k: ber(det, v) for k, v in a1.items()}
    for k in b0:
        print(f"{k:42s} plain {b0[k]:6.2f} %   filter-aware {b1[k]:6.2f} %")
    m0, m1 = float(np.mean(list(b0.values()))), float(np.mean(list(b1.values())))
    audio = np.stack(clips)
    print(f"clean BER plain {clean0:.2f} % / filter-aware {clean1:.2f} %; mean over the six: plain {m0:.2f} % / aware {m1:.2f} %; "
          f"SNR against the host: plain {snr_db(audio, y0):.1f} dB / aware {snr_db(audio, y1):.1f} dB")
    assert clean0 == 0.0 and clean1 == 0.0
    assert m0 >= 10.0
    assert m1 <= 0.5 * m0
