"""The general-geometry STFT path (csrc/stft_any.hip) on the GPU: the STFT / ISTFT plug-ins at any supported n_fft, hop and
win_length against torch.stft / torch.istft in float64 on the CPU (the calls the reference makes, utils/audio/stft.py:27-28,
:47-48), their backward against torch autograd, the card geometry on the general kernels against the card kernels, and the
refusals (NOLA, the loop's entry points)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from aware_amd._lib import require_gpu
    require_gpu()
    from aware_amd import runtime
    return runtime


def _win(window, win, dtype=torch.float64):
    return (torch.hann_window if window == "hann" else torch.hamming_window)(win, dtype=dtype)


def ref_stft(x, n_fft, hop, win, window):
    x = torch.as_tensor(x).double().cpu()
    return torch.stft(x, n_fft, hop, win, _win(window, win), center=True, pad_mode="reflect", return_complex=True)


def ref_istft(X, n_fft, hop, win, window, dtype=torch.float64):
    X = torch.as_tensor(X).cpu().to(torch.complex128 if dtype == torch.float64 else torch.complex64)
    return torch.istft(X, n_fft, hop, win, _win(window, win, dtype), center=True)


def unit_peak(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g)
    return (x / x.abs().max()).float()


def check_stft(mine, ref, what):
    mine = mine.detach().cpu().to(torch.complex128)
    assert mine.shape == ref.shape, (what, mine.shape, ref.shape)
    err = float((mine - ref).abs().max() / ref.abs().max())
    assert err <= 1e-5, (what, err)
    return err


def test_default_plugins_match_torch(rt):
    """STFT() / ISTFT() with the reference's own defaults (2048 / 512 / 2048): the card-only native layer refused them."""
    from aware_amd.utils.audio import STFT, ISTFT
    x = unit_peak(48000, 1)
    S = STFT()(x.cuda())
    ref = ref_stft(x, 2048, 512, 2048, "hann")
    check_stft(S, ref, "stft defaults")
    y = ISTFT()(S).cpu().double()
    yref = ref_istft(ref, 2048, 512, 2048, "hann")
    assert y.shape == yref.shape == (512 * (ref.shape[1] - 1),)
    assert float((y - yref).abs().max()) <= 2e-6
    assert float((y - x.double()[: y.numel()]).abs().max()) <= 2e-6


def test_win_length_is_honoured(rt):
    from aware_amd.utils.audio import STFT
    x = unit_peak(16000, 2)
    S = STFT(1024, 256, "hann", 512)(x.cuda())
    check_stft(S, ref_stft(x, 1024, 256, 512, "hann"), "win_length 512")


def _geometries():
    out = []
    for n_fft in (256, 512, 1024, 2048, 4096):
        hops = [n_fft // 8, n_fft // 4, n_fft // 2, n_fft, 3 * n_fft // 8 + 1]
        wins = [n_fft, n_fft // 2, n_fft // 2 + 1]
        i = 0
        for hop in hops:
            for win in wins:
                out.append((n_fft, hop, win, "hann" if i % 2 == 0 else "hamming"))
                i += 1
    return out


@pytest.mark.parametrize("geom", _geometries(), ids=lambda g: "-".join(map(str, g)))
def test_geometry_grid_ragged(rt, geom):
    """Ragged batches (clips just above n_fft/2 up to 10 s) through the runtime layer: aware_stft against torch.stft per clip,
    aware_istft of torch's spectrum against torch.istft (float64) where torch accepts the geometry, held to the larger of
    2e-6 and four times what torch itself reaches in float32 (a sparse window's small envelope amplifies rounding)."""
    n_fft, hop, win, window = geom
    plan = rt.Plan(n_fft, hop, win, window, general=True)        # (the grid holds the card geometry too)
    assert plan.general and plan.spectrum_stride == ((n_fft // 2 + 1 + 7) // 8) * 8
    lengths = [n_fft // 2 + 1, n_fft // 2 + 5, 16000 + 123, 160000]
    clips = [unit_peak(n, 10 + i) for i, n in enumerate(lengths)]
    batch = rt.Batch(lengths, plan=plan)
    spec = rt.stft(plan, batch, batch.pack(clips))
    F = n_fft // 2 + 1
    refs = []
    for i, c in enumerate(clips):
        ref = ref_stft(c, n_fft, hop, win, window)
        refs.append(ref)
        rows = spec[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :F].T
        check_stft(rows, ref, (geom, lengths[i]))
        assert float(spec[batch.frame_offsets[i]: batch.frame_offsets[i + 1], F:].abs().max()) == 0.0     # padding columns
    ok = all(rt.nola_ok(n_fft, hop, win, window, n) for n in lengths)
    if hop > win:
        assert not ok
    if not ok:
        with pytest.raises(RuntimeError, match="NOLA"):
            rt.istft(plan, batch, spec)
        return
    full = torch.zeros_like(spec)
    for i, ref in enumerate(refs):
        full[batch.frame_offsets[i]: batch.frame_offsets[i + 1], :F] = ref.T.to(torch.complex64).cuda()
    y = rt.istft(plan, batch, full).cpu().double()
    for i, ref in enumerate(refs):
        yi = y[batch.out_offsets[i]: batch.out_offsets[i] + batch.out_lengths[i]]
        if ref.shape[1] == 1:            # one frame: no output samples (torch.istft cannot reduce its empty envelope)
            assert yi.numel() == 0
            continue
        yref = ref_istft(ref, n_fft, hop, win, window)
        y32 = ref_istft(ref.to(torch.complex64), n_fft, hop, win, window, torch.float32).double()
        assert yi.shape == yref.shape
        tol = max(2e-6, 4 * float((y32 - yref).abs().max()))
        err = float((yi - yref).abs().max())
        assert err <= tol, (geom, lengths[i], err, tol)


def test_two_dimensional_input(rt):
    from aware_amd.utils.audio import STFT, ISTFT
    x = torch.stack([unit_peak(20000, 30 + b) for b in range(3)])
    S = STFT(512, 128, "hamming", 400)(x.cuda())
    ref = torch.stft(x.double(), 512, 128, 400, _win("hamming", 400), center=True, return_complex=True)
    assert S.shape == ref.shape
    for b in range(3):
        check_stft(S[b], ref[b], ("row", b))
    y = ISTFT(512, 128, "hamming", 400)(S)
    assert y.shape == (3, 128 * (ref.shape[-1] - 1))
    assert float((y.cpu().double() - x.double()[:, : y.shape[1]]).abs().max()) <= 2e-6
    # card geometry: rows are clips too
    Sc = STFT(1024, 256, "hann", 1024)(x.cuda())
    refc = torch.stft(x.double(), 1024, 256, 1024, _win("hann", 1024), center=True, return_complex=True)
    for b in range(3):
        check_stft(Sc[b], refc[b], ("card row", b))


def _chain_grad(x, n_fft, hop, win, window, scale, w_out, mine):
    from aware_amd.utils.audio import STFT, ISTFT, WaveformNormalizer, STFTDecomposer, STFTAssembler
    if mine:
        xd = x.cuda().requires_grad_(True)
        v = WaveformNormalizer()(xd)
        mag, ph = STFTDecomposer()(STFT(n_fft, hop, window, win)(v))
        y = WaveformNormalizer()(ISTFT(n_fft, hop, window, win)(STFTAssembler()(mag * scale.cuda(), ph)))
        (y * w_out.cuda()).sum().backward()
        return y.detach().cpu().double(), xd.grad.cpu().double()
    xr = x.double().requires_grad_(True)
    v = xr / torch.amax(torch.abs(xr) + 1e-8)
    S = torch.stft(v, n_fft, hop, win, _win(window, win), center=True, pad_mode="reflect", return_complex=True)
    m, p = torch.abs(S), torch.angle(S)
    y = torch.istft((m * scale.double()) * torch.exp(1j * p), n_fft, hop, win, _win(window, win), center=True)
    y = y / torch.amax(torch.abs(y) + 1e-8)
    (y * w_out.double()).sum().backward()
    return y.detach(), xr.grad


@pytest.mark.parametrize("geom", [(2048, 512, 2048, "hann"), (512, 128, 400, "hann")])
def test_reference_chain_backward_matches_autograd(rt, geom):
    """WaveformNormalizer -> STFT -> STFTDecomposer -> scale the band -> STFTAssembler -> ISTFT -> WaveformNormalizer, the
    reference's plug-in chain, at non-card geometries: output and input gradient against torch autograd in float64."""
    n_fft, hop, win, window = geom
    g = torch.Generator().manual_seed(n_fft + hop)
    x = (0.1 * torch.randn(16000 * 2 + 77, generator=g)).float()
    F = n_fft // 2 + 1
    scale = torch.ones(F, 1)
    scale[F // 16: F // 4] = 1.5
    T = 1 + x.numel() // hop
    w_out = torch.randn(hop * (T - 1), generator=g).float()
    y, gx = _chain_grad(x, n_fft, hop, win, window, scale, w_out, True)
    yr, gr = _chain_grad(x, n_fft, hop, win, window, scale, w_out, False)
    assert float((y - yr).abs().max()) <= 3e-6
    rel = float((gx - gr).norm() / gr.norm())
    assert rel <= 2e-5, rel


def test_stft_backward_2d_and_istft_backward(rt):
    from aware_amd.utils.audio import STFT, ISTFT
    g = torch.Generator().manual_seed(7)
    x = (0.1 * torch.randn(2, 9000, generator=g)).float()
    cot = torch.randn(2, 257, 1 + 9000 // 96, dtype=torch.complex64, generator=g)
    xd = x.cuda().requires_grad_(True)
    S = STFT(512, 96, "hann", 512)(xd)
    (S.real * cot.real.cuda() + S.imag * cot.imag.cuda()).sum().backward()
    xr = x.double().requires_grad_(True)
    Sr = torch.stft(xr, 512, 96, 512, _win("hann", 512), center=True, return_complex=True)
    (Sr.real * cot.real.double() + Sr.imag * cot.imag.double()).sum().backward()
    assert float((xd.grad.cpu().double() - xr.grad).norm() / xr.grad.norm()) <= 2e-6
    X = Sr.detach().to(torch.complex64)
    Xd = X.cuda().requires_grad_(True)
    y = ISTFT(512, 96, "hann", 512)(Xd)
    w = torch.randn(y.shape, generator=g)
    (y * w.cuda()).sum().backward()
    Xr = X.to(torch.complex128).requires_grad_(True)
    yr = torch.istft(Xr, 512, 96, 512, _win("hann", 512), center=True)
    (yr * w.double()).sum().backward()
    gd, gref = Xd.grad.cpu().to(torch.complex128), Xr.grad
    assert float((gd - gref).abs().max() / gref.abs().max()) <= 2e-6


def test_card_geometry_on_general_kernels(rt):
    """AWARE_PLAN_GENERAL on the card geometry against the card kernels: all four transforms agree to 2e-6 relative; the
    card plan itself stays the card plan."""
    card, gen = rt.Plan(), rt.Plan(general=True)
    assert not card.general and card.spectrum_stride == rt.FULL_STRIDE == 520
    assert gen.general and gen.spectrum_stride == 520
    lengths = [16000, 48000, 777, 23456]
    clips = [unit_peak(n, 50 + i) for i, n in enumerate(lengths)]
    bc, bg = rt.Batch(lengths), rt.Batch(lengths, plan=gen)
    assert bc.frames == bg.frames and bc.out_offsets == bg.out_offsets
    a = bc.pack(clips)
    for norm in (False, True):
        sc, sg = rt.stft(card, bc, a, normalize=norm), rt.stft(gen, bg, a, normalize=norm)
        assert float((sc[:, :513] - sg[:, :513]).abs().max() / sc[:, :513].abs().max()) <= 2e-6
    spec = rt.stft(card, bc, a)
    yc, yg = rt.istft(card, bc, spec), rt.istft(gen, bg, spec)
    assert float((yc - yg).abs().max() / yc.abs().max()) <= 2e-6
    yc, yg = rt.istft(card, bc, spec, normalize=True), rt.istft(gen, bg, spec, normalize=True)
    assert float((yc - yg).abs().max()) <= 2e-6
    g = torch.Generator().manual_seed(9)
    G = torch.zeros(bc.total_frames, 520, dtype=torch.complex64)
    G[:, :513] = torch.complex(torch.randn(bc.total_frames, 513, generator=g), torch.randn(bc.total_frames, 513, generator=g))
    G = G.cuda()
    gc, gg = rt.stft_bwd(card, bc, G), rt.stft_bwd(gen, bg, G)
    assert float((gc - gg).abs().max() / gc.abs().max()) <= 2e-6
    ga = torch.randn(bc.total_out, generator=g).cuda()
    hc, hg = rt.istft_bwd(card, bc, ga), rt.istft_bwd(gen, bg, ga)
    assert float((hc[:, :513] - hg[:, :513]).abs().max() / hc[:, :513].abs().max()) <= 2e-6


def test_nola_violation_raises(rt):
    from aware_amd.utils.audio import STFT, ISTFT
    x = unit_peak(16000, 3)
    S = STFT(1024, 512, "hann", 256)(x.cuda())          # the STFT direction accepts it, as torch does
    check_stft(S, ref_stft(x, 1024, 512, 256, "hann"), "nola stft")
    with pytest.raises(RuntimeError, match="NOLA"):
        ISTFT(1024, 512, "hann", 256)(S)
    with pytest.raises(RuntimeError):
        torch.istft(S.cpu(), 1024, 512, 256, _win("hann", 256, torch.float32), center=True)


def test_loop_entry_points_refuse_general_plans(rt):
    lib = rt.load_library()
    gen = rt.Plan(2048, 512, 2048, "hann")
    bg = rt.Batch([16000], plan=gen)
    card = rt.Plan()
    bc = rt.Batch([16000])
    dummy = C.c_void_p(16)
    audio = torch.zeros(16000, device="cuda")
    assert lib.aware_stft_band(gen.h, bg.h, rt._ptr(audio), 0, dummy, dummy, dummy, None) == -2
    ch = (C.c_int * 5)(128, 512, 1024, 1024, 40)
    w = (C.c_void_p * 4)(dummy, dummy, dummy, dummy)
    h = C.c_void_p()
    mel = np.zeros(128 * 1025, dtype=np.float32)
    assert lib.aware_detector_create(C.byref(h), gen.h, mel.ctypes.data_as(C.c_void_p), 128, 4, ch, w, w) == -2
    assert lib.aware_detect(gen.h, dummy, bg.h, rt._ptr(audio), dummy, dummy, 1, None) == -2
    cfg = rt.EmbedConfig()
    assert lib.aware_embed_create(C.byref(h), gen.h, dummy, bg.h, C.byref(cfg), dummy, 1, None) == -2
    # a batch that was not built for the plan
    spec = torch.empty(bc.total_frames, 1032, dtype=torch.complex64, device="cuda")
    assert lib.aware_stft(gen.h, bc.h, rt._ptr(audio), 0, rt._ptr(spec), None, None) == -1
    assert lib.aware_stft(card.h, bg.h, rt._ptr(audio), 0, rt._ptr(spec), None, None) == -1
    other = rt.Plan(2048, 256, 2048, "hann")
    assert lib.aware_stft(other.h, bg.h, rt._ptr(audio), 0, rt._ptr(spec), None, None) == -1
    torch.cuda.synchronize()
