"""Attack-aware embedding on the general route (aware_embed_set_general_chain, csrc/loop_any_chain.hip)
on the device, against the restatement of tests/test_general_chain_host.py (AttackedGeneralLoop) and, at the card geometry,
against the card route with the same chain and seeds.

Geometries: G1 256 / 64 / 256, G2 512 / 200 / 400 hamming, H75 256 / 75 / 256 (an odd hop: odd offsets and lengths), G3 the
card's with both keys, G4 2048 / 512 / 2048 at 44.1 kHz.  The kernels cut a clip into pieces of P = 3072 samples, so the clips
are chosen around P: Ny one hop below P (the largest multiple of the hop below it), Ny = P where the hop divides it, the first
multiple above P, several pieces and a remainder, and the shortest clip the route takes (n_fft/2 + 1 samples).  Batch A holds
the shortest clip, so its suppression is 64 samples; batch B holds none, and its suppression is long enough to cross a piece
boundary (asserted from the draws).  At H75 the two batches hold Ny % 4 = 0, 1, 2 and 3.

Run on the MI355X box:  python -m pytest tests/test_gpu_general_chain.py -m gpu -q -s
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import make_clip
from loop_support import CHAIN_BOUND, O, LA, attacked, ex_entries, norm2, rt, sampled, synthesis  # noqa: F401
from test_general_chain_host import CLAIMS, AttackedGeneralLoop, claim
from test_gpu_general_geometry import GEOM, lengths_of

pytestmark = pytest.mark.gpu

P = 3072
GEOMS = {k: GEOM[k] for k in ("G1", "G2", "G3", "G4")}
GEOMS["H75"] = (256, 75, 256, "hann", 16000, (500, 4000), 16000)


def ny_around_p(hop):
    """(below, exact or None, above): multiples of the hop around the piece length"""
    below = P - hop if P % hop == 0 else hop * (P // hop)
    return below, (P if P % hop == 0 else None), hop * (P // hop) + hop


def lengths_for(name, which):
    """Input lengths n (Ny = hop * (n // hop)) of batch A (with the shortest clip), B (without), U (uniform, eight)."""
    n_fft, hop = GEOMS[name][:2]
    below, exact, above = ny_around_p(hop)
    several = hop * ((5 * P // 2) // hop + 1)          # two pieces and a remainder
    tail = hop // 3                                    # samples the framing drops
    ny = {"A": [several, below, None, above],
          "B": [exact or below, above + hop, above + 2 * hop, several + 2 * hop],
          "U": [several + 2 * hop] * 8}[which]
    return [n_fft // 2 + 1 if m is None else m + tail for m in ny]


def chains(sr, k):
    """The chains of the issue at sample rate sr with a suppression of k samples."""
    sup = {"kind": "sample_suppression", "seconds": (k + 0.5) / sr}
    noise = {"kind": "gaussian_noise", "snr_db": 10.0}
    env64 = {"kind": "gain_envelope", "period": 64.5 / sr, "floor": 0.25}
    env = {"kind": "gain_envelope", "period": [0.05, 0.5], "prob": 0.75}
    return {"noise": [noise], "suppression": [sup], "envelope 64": [env64], "envelope": [env], "suppression + noise": [sup, noise],
            "noise + suppression": [noise, dict(sup, prob=0.75)], "four": [env, sup, noise, env64]}


_CASES = {}


def case(rt, name):
    """Embedder (no chain), plan and device detector of a geometry: built once, shared, never modified."""
    if name not in _CASES:
        from aware_amd.embedding import AWAREEmbedder
        n_fft, hop, win, window, sr, band, _ = GEOMS[name]
        emb = AWAREEmbedder(frame_length=n_fft, hop_length=hop, win_length=win, window=window, embedding_bands=band,
                            general_geometry=True, verbose=False, loss="push_extremes", use_graph=False,
                            detection_net_cfg={"n_fft": n_fft, "sample_rate": sr})
        plan = emb._plan(sr)
        _CASES[name] = dict(emb=emb, plan=plan, dev=emb.detection_net.device_weights(plan), sr=sr)
    return _CASES[name]


def clips_for(lengths, seed0=300):
    pairs = [make_clip(seed0 + i, n) for i, n in enumerate(lengths)]
    return [p[0] for p in pairs], np.stack([(2 * p[1] - 1).astype(np.float32) for p in pairs])


def session(rt, name, lengths, chain=None, seeds=None, seed0=300, **kw):
    """A begun session on make_clip(seed0 + i, n) clips, with `chain` set through set_general_chain (None: never set)."""
    c = case(rt, name)
    batch = c["emb"].make_batch(lengths, c["sr"])
    clips, wm = clips_for(lengths, seed0)
    sess = rt.EmbedSession(c["plan"], c["dev"], batch, **kw)
    if chain is not None:
        sess.set_general_chain(chain, seeds if seeds is not None else list(range(batch.B)), c["sr"])
    sess.begin(batch.pack(clips), torch.from_numpy(wm).cuda())
    return sess, batch, clips, wm


def loop64(name, chain, seed):
    n_fft, hop, win, window, sr, band, _ = GEOMS[name]
    return AttackedGeneralLoop(chain, [seed], n_fft, hop, win, window, sr, band, dtype=torch.float64)


def trivial(name, n):
    """one pooled frame and a synthesis torch.stft cannot pad: values 0, loss 1, gradient 0 (tests/test_gpu_general_geometry.py)"""
    n_fft, hop = GEOMS[name][:2]
    return (1 + n // hop) // 2 == 1 and hop * (n // hop) <= n_fft // 2


# ---- forward ----------------------------------------------------------------------------------------------------------------------------
def check_forward(LA, sess, batch, chain, seeds, step, sr, tag):
    """Buffer 12 against apply_chain(N(N(buffer 9))) in float64: zeros exactly where the restatement has them, every other sample
    within 1e-6 of the unit peak (CHAIN_BOUND of the reference's peak for a chain with an envelope), the card tests' bounds."""
    torch.cuda.synchronize()
    chain = LA.parse_chain(chain, sr)
    env = any(a["kind"] == "gain_envelope" for a in chain)
    worst = 0.0
    for b, y, z in sampled(sess, batch):
        ref = LA.apply_chain(norm2(y.double())[None], chain, [seeds[b]], step, sr)[0]
        assert len(z) == batch.out_lengths[b] and bool(torch.isfinite(z).all()), (tag, step, b)
        np.testing.assert_array_equal((z == 0).numpy(), (ref == 0).numpy(), err_msg=f"{tag} step {step} clip {b}")
        worst = max(worst, float((z.double() - ref).abs().max()) / (float(ref.abs().max()) if env else 1.0))
    print(f"{tag}, step {step}: max |z - restatement| = {worst:.2e} (bound {CHAIN_BOUND if env else 1e-6:.2e})")
    assert worst < (CHAIN_BOUND if env else 1e-6), (tag, step, worst)


def crossings(LA, chain, seeds, steps, out_lengths, sr):
    """how often a firing suppression of the chain covers a piece boundary"""
    chain, n = LA.parse_chain(chain, sr), 0
    for j, a in enumerate(chain):
        if a["kind"] != "sample_suppression":
            continue
        k = LA.suppression_samples(a, sr)
        for seed, ny in zip(seeds, out_lengths):
            for s in steps:
                r = LA.entry_draw(seed, s, j)
                start = LA.suppression_start(r[1], ny, k)
                n += int(LA.fires(r[0], a["prob"]) and start // P != (start + k - 1) // P)
    return n


@pytest.mark.parametrize("which", ["A", "B", "U"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_forward_matches_the_restatement(rt, LA, name, which):
    """forward_at_steps_0_2_17 on the general route: every chain of the issue, at step 0 (after gradient()), 2 and 17."""
    sr = GEOMS[name][4]
    lengths = lengths_for(name, which)
    k = 64 if which == "A" else 2000
    seeds = [11 + 3 * i for i in range(len(lengths))]
    for cname, chain in chains(sr, k).items():
        if which == "U" and cname != "four":
            continue
        sess, batch, _, _ = session(rt, name, lengths, chain, seeds, seed0=20, num_iterations=20)
        tag = f"{name} {which} {cname}"
        sess.gradient()
        check_forward(LA, sess, batch, chain, seeds, 0, sr, tag)
        assert int(sess.step.cpu()[0]) == 0                       # aware_embed_gradient does not advance the step
        z0 = sess.attacked.clone()
        sess.iterate(3)
        check_forward(LA, sess, batch, chain, seeds, 2, sr, tag)
        assert not torch.equal(z0, sess.attacked)
        sess.iterate(15)
        assert int(sess.step.cpu()[0]) == 18
        check_forward(LA, sess, batch, chain, seeds, 17, sr, tag)
        if which == "B" and "suppression" in cname:
            n = crossings(LA, chain, seeds, (0, 2, 17), batch.out_lengths, sr)
            print(f"{tag}: {n} suppressions across a piece boundary")
            assert n > 0, tag
    if name == "H75":                                             # Ny % 4 = 1, 2, 3 and clips at offsets that are no multiple of 4
        rem = {"A": {0, 1, 3}, "B": {0, 1, 2, 3}, "U": {3}}[which]
        assert {m % 4 for m in batch.out_lengths} == rem and any(o % 4 for o in batch.out_offsets), batch.out_lengths


# ---- first gradient, loss and prediction --------------------------------------------------------------------------------------------------
_REFS = {}


def reference(name, cname, chain, lengths, seeds):
    """float64 autograd over AttackedGeneralLoop per clip, once per (geometry, chain)"""
    if (name, cname) not in _REFS:
        clips, wm = clips_for(lengths)
        out = []
        for clip, w, n, seed in zip(clips, wm, lengths, seeds):
            if trivial(name, n):
                out.append(None)
                continue
            loss, pred, g = loop64(name, chain, seed).first_iteration(torch.from_numpy(clip).double()[None], torch.from_numpy(w).double()[None])
            out.append((float(loss[0]), pred[0].numpy(), g[0].T.contiguous()))
        _REFS[(name, cname)] = out
    return _REFS[(name, cname)]


@pytest.mark.parametrize("pipe", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_first_step(rt, name, pipe):
    """Loss, prediction and aware_embed_gradient of the first loop body against float64 autograd over AttackedGeneralLoop, batch A,
    on both conv pipes.  Bounds of tests/test_gpu_general_geometry.py::test_first_step: loss 5e-5 * max(1, |loss|), gradient
    relative L2 2e-4 on bf16x3 and 2e-3 on f16x2; the prediction within the 1e-4 its test_detect holds the same values to.  (That
    file has no exception for a LeakyReLU argument at its kink, so none is made here.)  The shortest clip reads loss 1 and a
    gradient of exactly 0."""
    sr = GEOMS[name][4]
    lengths = lengths_for(name, "A")
    seeds = [5 + 2 * i for i in range(len(lengths))]
    bar = {"bf16x3": 2e-4, "f16x2": 2e-3}[pipe]
    all_chains = chains(sr, 64)
    for cname in ("suppression + noise", "four", "noise + suppression"):
        chain = all_chains[cname]
        ref = reference(name, cname, chain, lengths, seeds)
        sess, batch, _, _ = session(rt, name, lengths, chain, seeds, use_graph=False, conv_pipe=pipe)
        g = sess.gradient()
        torch.cuda.synchronize()
        g, loss, pred = g.cpu().double(), sess.loss.cpu().numpy().copy(), sess.pred.cpu().numpy().copy()
        nb = case(rt, name)["plan"].nband
        assert torch.isfinite(g).all() and np.isfinite(loss).all()
        figures = []
        for i, r in enumerate(ref):
            r0, r1 = batch.frame_offsets[i], batch.frame_offsets[i + 1]
            if r is None:
                print(f"{name} {pipe} {cname} clip {i} (n = {lengths[i]}): loss {float(loss[i])!r} (must be 1), max |g| {float(g[r0:r1].abs().max()):.1e} (must be 0)")
                figures.append((i, abs(float(loss[i]) - 1.0), float(np.abs(pred[i]).max()), float(g[r0:r1].abs().max()), True))
                continue
            el = abs(float(loss[i]) - r[0]) / max(1.0, abs(r[0]))
            ep = float(np.abs(pred[i] - r[1]).max())
            rel = float((g[r0:r1, :nb] - r[2]).norm() / r[2].norm())
            figures.append((i, el, ep, rel, False))
            print(f"{name} {pipe} {cname} clip {i} (n = {lengths[i]}): loss err {el:.1e} (bound 5e-5), pred err {ep:.1e} (bound 1e-4), "
                  f"gradient rel L2 {rel:.2e} (bound {bar:.0e})")
        for i, el, ep, rel, zero in figures:
            assert (el == 0.0 and ep == 0.0 and rel == 0.0) if zero else (el < 5e-5 and ep < 1e-4 and rel < bar), (name, pipe, cname, i, el, ep, rel)


# ---- G3 against the card route --------------------------------------------------------------------------------------------------------------
def card_session(rt, O, lengths, chain, seeds, **kw):
    clips, wm = clips_for(lengths)
    plan = rt.Plan()
    ws, bs = O.detector_weights()
    det = rt.DetectorWeights(plan, O.mel_filter_bank(), [w.numpy() for w in ws], [b.numpy() for b in bs])
    batch = rt.Batch(lengths)
    sess = rt.EmbedSession(plan, det, batch, **kw)
    if chain:
        sess.set_loop_attacks(chain, seeds)
    sess.begin(batch.pack(clips), torch.from_numpy(wm).cuda())
    return sess, batch


def run5(sess):
    g = sess.gradient().cpu()
    z = sess.attacked.cpu().clone() if sess.attacked is not None else None
    losses = []
    for _ in range(5):
        sess.iterate(1)
        losses.append(sess.loss.cpu().clone())
    return g, z, torch.stack(losses)


def compare_routes(tag, batch, a, b):
    """first gradient relative L2 per clip, five losses: section 31's bounds between the two routes (2e-4 on bf16x3, 1e-3)"""
    rel = []
    for i in range(batch.B):
        r0, r1 = batch.frame_offsets[i], batch.frame_offsets[i + 1]
        x, y = a[0][r0:r1, :225].double(), b[0][r0:r1, :225].double()
        rel.append(float(x.abs().max()) if float(y.norm()) == 0.0 else float((x - y).norm() / y.norm()))
    dl = float((a[2] - b[2]).abs().max())
    print(f"{tag}: first gradient rel L2 per clip {['%.1e' % r for r in rel]} (bound 2e-4), five losses {dl:.1e} (bound 1e-3)")
    assert max(rel) < 2e-4 and dl < 1e-3, (tag, rel, dl)


@pytest.mark.parametrize("cname", ["suppression + noise", "four"])
def test_card_geometry_against_the_card_route(rt, O, cname):
    """G3 with the same chain and seeds on both routes: buffer 12 within 2e-6 (each route's 1e-6 against the restatement), the
    first gradient to 2e-4 relative L2 on bf16x3, five losses within 1e-3."""
    lengths = lengths_for("G3", "A")
    chain = chains(16000, 64)[cname]
    seeds = [7, 8, 9, 10]
    kw = dict(num_iterations=5, use_graph=False, conv_pipe="bf16x3")
    card, cb = card_session(rt, O, lengths, chain, seeds, **kw)
    gen, batch, _, _ = session(rt, "G3", lengths, chain, seeds, **kw)
    assert batch.out_offsets == cb.out_offsets and batch.out_lengths == cb.out_lengths
    a, b = run5(gen), run5(card)
    dz = float((a[1] - b[1]).abs().max())
    print(f"G3 {cname}: buffer 12 of the two routes at step 0 max |diff| {dz:.1e} (bound 2e-6)")
    assert dz < 2e-6
    compare_routes(f"G3 {cname}", batch, a, b)


# ---- graph replay -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["G1", "H75", "G4"])
def test_graph_replay_is_eager_bit_for_bit(rt, name):
    """20 steps under graph replay and eager: coefficients, best coefficients, best losses and, after every step, the losses and
    buffer 12, bit for bit; z differs from step to step (the step is read from device memory)."""
    sr = GEOMS[name][4]
    lengths = lengths_for(name, "B")
    chain = chains(sr, 2000)["four"]
    out = []
    for use_graph in (True, False):
        sess, batch, _, _ = session(rt, name, lengths, chain, num_iterations=20, use_graph=use_graph)
        ls, zs = [], []
        for _ in range(20):
            sess.iterate(1)
            ls.append(sess.loss.clone())
            zs.append(sess.attacked.clone())
        torch.cuda.synchronize()
        assert int(sess.step.cpu()[0]) == 20
        out.append((sess.coef.cpu(), sess.best_coef.cpu(), sess.best_loss.cpu(), torch.stack(ls).cpu(), torch.stack(zs).cpu()))
    for what, a, b in zip(("coef", "best_coef", "best_loss", "loss", "z"), *out):
        assert torch.equal(a, b), (name, what, float((a.double() - b.double()).abs().max()))
    z = out[0][4]
    assert all(not torch.equal(z[s], z[s + 1]) for s in range(19))


# ---- prob 0, never set, cleared -----------------------------------------------------------------------------------------------------------------
def test_prob_0_is_the_plain_general_route_to_the_routes_bounds(rt):
    """Every entry with prob 0 at G2, batch A: the first gradient and five losses against the chain-free session within the bounds
    between the two routes at G3 (2e-4 relative L2, 1e-3).  The two extra normalisers move the signal by an ulp, so the two are
    not bit for bit.  Measured: first gradient 2.4e-6 relative L2 at most, five losses within 1.2e-7."""
    lengths = lengths_for("G2", "A")
    chain = [dict(a, prob=0.0) for a in chains(16000, 64)["four"]]
    kw = dict(num_iterations=5, use_graph=False, conv_pipe="bf16x3")
    att, batch, _, _ = session(rt, "G2", lengths, chain, **kw)
    plain, _, _, _ = session(rt, "G2", lengths, None, **kw)
    a, b = run5(att), run5(plain)
    for z, y in zip(attacked(att, batch), synthesis(att, batch)):
        assert float((z.double() - norm2(y.double())).abs().max()) < 2e-7
    compare_routes("G2 prob 0 against no chain", batch, a, b)


def plain_run(rt, name, lengths, how):
    """detect values, first gradient, five losses and the output of a session whose chain was never set / set and cleared"""
    c = case(rt, name)
    sess, batch, clips, _ = session(rt, name, lengths, None, num_iterations=5, use_graph=False)
    if how == "cleared":
        sess2 = rt.EmbedSession(c["plan"], c["dev"], batch, num_iterations=5, use_graph=False)
        sess2.set_general_chain(chains(c["sr"], 64)["four"], list(range(batch.B)), c["sr"])
        assert sess2.attacked is not None
        sess2.set_general_chain([], [], c["sr"])
        assert sess2.attacked is None
        sess2.begin(sess._audio, sess._target)
        sess = sess2
    g, _, losses = run5(sess)
    from aware_amd.detection import AWAREDetector
    n_fft, hop, win, window, sr, band, _ = GEOMS[name]
    det = AWAREDetector(c["emb"].detection_net, frame_length=n_fft, hop_length=hop, win_length=win, window=window,
                        embedding_bands=band, general_geometry=True)
    return det.detect_batch(clips, sr).cpu(), g, losses, sess.finish().cpu()


def test_never_set_and_cleared_keep_the_plain_routes_bits(rt):
    """A session whose chain was never set, and one whose chain was set and then cleared with n_attacks = 0, launch what the plain
    general route launches: detect values, first gradient, five losses and output bit for bit, and within the plain route's own
    bounds of the float64 restatement (tests/test_gpu_general_geometry.py holds the parent's route to the same)."""
    lengths = lengths_of("G2")
    never, cleared = plain_run(rt, "G2", lengths, "never"), plain_run(rt, "G2", lengths, "cleared")
    for what, a, b in zip(("detect", "gradient", "losses", "output"), never, cleared):
        assert torch.equal(a, b), what
    # ... and the chain-free session is the one tests/test_gpu_general_geometry.py checks against the restatement: same lengths,
    # same clips (make_clip(300 + i, n)), so its test_first_step and test_trajectory cover these bits


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_error_codes_and_workspace(rt, O):
    lengths = lengths_for("H75", "A")
    sess, batch, _, _ = session(rt, "H75", lengths, None, num_iterations=3, use_graph=False)
    lib = sess.lib
    NO, SU, EV = (0, 1.0, [10.0]), (1, 1.0, [64.0]), (8, 0.75, [800.0, 8000.0, 0.25])
    size = lambda ent: lib.aware_embed_general_chain_workspace_bytes(batch.h, ex_entries(ent), len(ent))
    np_ = -(-max(batch.out_lengths) // P)
    want, off = 0, 0
    for count, item in ((batch.total_out, 4), (batch.B * np_, 8), (4 * batch.B * np_, 8), (batch.B * np_, 8), (batch.B * np_, 8), (batch.B, 4)):
        off = ((off + 255) & ~255) + count * item
    nb = size([NO])
    assert nb == off == size([EV, SU, NO, EV]) and size([]) == 0 and size([NO] * 5) == 0
    ws = torch.empty(nb + 256, dtype=torch.uint8, device="cuda")
    sd = (C.c_uint32 * batch.B)(*range(batch.B))

    def call(ent, n=None, seeds=sd, wsp=ws.data_ptr(), wsb=nb, h=sess.h):
        return lib.aware_embed_set_general_chain(h, ex_entries(ent) if ent is not None else None, len(ent) if n is None else n, seeds,
                                                 C.c_void_p(wsp), wsb, None)

    assert call([NO], wsb=nb - 1) == -4 and not lib.aware_embed_buffer(sess.h, 12)
    assert call([NO], wsp=ws.data_ptr() + 4) == -1 and call(None, n=1) == -1 and call([NO], seeds=None) == -1
    assert call([NO] * 5) == -1 and call([NO], n=-1) == -1 and call([(0, 1.5, [10.0])]) == -1 and call([(8, 1.0, [32.0, 64.0, 0.0])]) == -1
    for kind, p in ((2, [1600.0, 8000.0, -3.0]), (3, [-3678.0, 3896.0]), (7, [1.0, 32.0, 0.0]), (12, [-100.0, 100.0, 0.0, 0.0])):
        assert call([NO, (kind, 1.0, p)]) == -2, kind
    assert call([(1, 1.0, [float(min(batch.out_lengths))])]) == -2           # k >= Ny of the shortest clip
    assert not lib.aware_embed_buffer(sess.h, 12)                            # nothing was set by a refused call
    assert call([EV, SU, NO, EV]) == 0 and lib.aware_embed_buffer(sess.h, 12) and not lib.aware_embed_buffer(sess.h, 13)
    assert call([], n=0) == 0 and not lib.aware_embed_buffer(sess.h, 12)
    assert call([NO]) == 0
    sess.iterate(1)
    assert call([NO]) == -1 and call([], n=0) == -1                          # after the first iterate
    # the old setters still refuse a general session; the new one refuses a card session
    fresh, _, _, _ = session(rt, "H75", lengths, None, num_iterations=3, use_graph=False)
    with pytest.raises(Exception, match="unsupported"):
        fresh.set_loop_attacks([{"kind": "gaussian_noise", "snr_db": 10.0}], [0] * batch.B)
    with pytest.raises(Exception, match="unsupported"):
        fresh.set_loop_attacks([{"kind": "gain_envelope", "period": 0.05}], [0] * batch.B)
    with pytest.raises(Exception, match="unsupported"):
        fresh.set_loop_mixture([{"weight": 0.5, "chain": [{"kind": "gaussian_noise", "snr_db": 10.0}]}], [0] * batch.B)
    assert lib.aware_embed_loop_attack_workspace_bytes_ex(batch.h, ex_entries([NO]), 1) == 0
    card, cb = card_session(rt, O, [16000, 8000], None, None, num_iterations=3, use_graph=False)
    assert lib.aware_embed_general_chain_workspace_bytes(cb.h, ex_entries([NO]), 1) == 0
    assert call([NO], h=card.h) == -2 and call([], n=0, h=card.h) == -2
    with pytest.raises(NotImplementedError, match="speed_change"):
        fresh.set_general_chain([{"kind": "speed_change", "cents": 100.0}], [0] * batch.B)
    with pytest.raises(ValueError, match="clip 2"):
        fresh.set_general_chain([{"kind": "sample_suppression", "seconds": 0.1}], [0] * batch.B)      # check_lengths, before any launch
    torch.cuda.synchronize()


# ---- a registry optimiser -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore:Converting a tensor with requires_grad=True to a scalar")
def test_registry_optimizer_with_a_chain(rt):
    """Adam under a step schedule (own_step: launch_opt_rows behind band_coef_grad, the backward launches at step - 1) at G1
    through AWAREEmbedder with both keys, against the float32 restatement's torch.optim loop: per-step losses to 1e-3, the bound of
    tests/test_gpu_general_geometry.py::test_registry_optimizer_on_the_general_route."""
    from aware_amd.embedding import AWAREEmbedder
    n = 6
    n_fft, hop, win, window, sr, band, _ = GEOMS["G1"]
    chain = chains(sr, 2000)["suppression + noise"]
    opt, sched = {"name": "adam", "params": {"lr": 0.05}}, {"name": "step", "params": {"step_size": 2, "gamma": 0.5}}
    emb = AWAREEmbedder(frame_length=n_fft, hop_length=hop, win_length=win, general_geometry=True, general_loop_attacks=True,
                        loop_attacks=chain, loop_attack_seed=3, num_iterations=n, verbose=False, use_graph=False, loss="push_extremes",
                        detection_net_cfg={"n_fft": n_fft}, optimizer_cfg=opt, scheduler_cfg=sched)
    length = lengths_for("G1", "B")[3]
    audio, bits = make_clip(3, length)
    wm = (2 * bits - 1).astype(np.float32)
    batch = emb.make_batch([length], sr)
    sess = emb.start_session(batch, sr)
    assert sess.attacked is not None
    sess.begin(batch.pack([audio]), torch.from_numpy(wm)[None].cuda())
    mine = []
    for _ in range(n):
        sess.iterate(1)
        mine.append(float(sess.loss.cpu()[0]))
    ref = []
    AttackedGeneralLoop(chain, [3], n_fft, hop, win, window, sr, band, num_iterations=n, optimizer="adam", optimizer_params=opt["params"],
                        scheduler="step", scheduler_params=sched["params"]).embed_registry(
        audio[None], wm[None], record=lambda it, l, lr: ref.append(l))
    d = np.abs(np.asarray(mine) - np.asarray(ref))
    print(f"Adam + step schedule with a chain: losses {np.round(mine, 5).tolist()}, max |mine - restatement| {d.max():.1e} (bound 1e-3)")
    assert d.max() < 1e-3, (mine, ref)


# ---- the value claim on the device ---------------------------------------------------------------------------------------------------------------
_VALUE = {}


def value_run(rt, chain_name):
    """Four make_clip(s, 44100) clips, 2048 / 512 / 2048 at 44.1 kHz, 400 steps through embed_batch; None: the plain embedding"""
    if chain_name not in _VALUE:
        from aware_amd.detection import AWAREDetector
        from aware_amd.embedding import AWAREEmbedder
        n_fft, hop, win, window, sr, band, _ = GEOMS["G4"]
        kw = dict(general_loop_attacks=True, loop_attacks=CLAIMS[chain_name][0]) if chain_name else {}
        emb = AWAREEmbedder(frame_length=n_fft, hop_length=hop, win_length=win, window=window, embedding_bands=band,
                            general_geometry=True, verbose=False, loss="push_extremes", num_iterations=400,
                            detection_net_cfg={"n_fft": n_fft, "sample_rate": sr}, **kw)
        det = AWAREDetector(emb.detection_net, frame_length=n_fft, hop_length=hop, win_length=win, window=window,
                            embedding_bands=band, general_geometry=True)
        pairs = [make_clip(s, sr) for s in range(4)]
        bits = np.stack([p[1] for p in pairs])
        outs = emb.embed_batch([p[0] for p in pairs], sr, 2.0 * bits - 1.0)
        _VALUE[chain_name] = (np.stack([o.cpu().numpy() for o in outs]), det, bits)
    return _VALUE[chain_name]


@pytest.mark.parametrize("name", list(CLAIMS))
def test_value_claim_on_the_device(rt, name):
    """The value claim of tests/test_general_chain_host.py through AWAREEmbedder(general_geometry=True, general_loop_attacks=True,
    loop_attacks=...) and detect_batch: clean 0 % for both embeddings, the plain mean at least 10 %, the aware mean at most half.
    Measured on the MI355X (plain mean -> aware mean): noise 27.81 -> 0.47 %, suppression 50.62 -> 0.00 %, gain curves
    39.38 -> 2.92 %; clean 0 % everywhere."""
    y0, det, bits = value_run(rt, None)
    y1, _, _ = value_run(rt, name)

    def ber(z):
        vals = det.detect_batch(list(np.asarray(z, dtype=np.float32)), 44100).cpu().numpy()
        return 100.0 * float(((vals > 0).astype(np.int32) != bits).mean())

    claim(name, ber, y0, y1)
