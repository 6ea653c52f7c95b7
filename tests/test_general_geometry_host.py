"""The embed / detect loop at any STFT geometry (key general_geometry), host side.

This file holds the geometry-generic restatement of the loop that tests/test_gpu_general_geometry.py compares the device
against: `GeneralLoop`, written on oracle.aware_oracle's stft, istft, band_indices, mel_filter_bank, Detector and Embedder
with the geometry, the window (centred and zero-padded for win_length < n_fft, as torch.stft does), the sample rate and the
band as arguments.  At the card geometry it is the oracle's Embedder bit for bit.  Then: the key at construction, the
refusals, the clip checks, the stride rule, and the claim that the loop works at other geometries (clean BER 0, mean |value|
far above what unmarked audio reads) at two of them on the CPU.
"""
import numpy as np
import pytest
import torch

from conftest import make_clip
from oracle import aware_oracle as O

# n_fft, hop, win_length, sample rate, clip length, band bins: the geometries the loop was measured at on the CPU
TABLE = [(1024, 256, 1024, 16000, 16000, 225), (512, 128, 512, 16000, 16000, 113), (256, 64, 256, 16000, 16000, 57),
         (1024, 128, 1024, 16000, 16000, 225), (1024, 256, 800, 16000, 16000, 225), (2048, 512, 2048, 16000, 16000, 449),
         (4096, 1024, 4096, 16000, 16000, 897), (2048, 512, 2048, 44100, 44100, 162)]
BAND = (500, 4000)


def padded_window(name, win_length, n_fft, dtype=torch.float32):
    """torch.hann_window / torch.hamming_window(win_length) (periodic), zero-padded to n_fft with (n_fft - win_length) // 2
    zeros on the left: what torch.stft and torch.istft make of a short window."""
    w = {"hann": torch.hann_window, "hamming": torch.hamming_window}[name](win_length, dtype=dtype)
    left = (n_fft - win_length) // 2
    return torch.nn.functional.pad(w, (left, n_fft - win_length - left))


class GeneralLoop(O.Embedder):
    """O.Embedder with the geometry as arguments: analyse, recompute_magnitude, embed and detect_raw restated with
    (n_fft, hop, window) handed to O.stft / O.istft, the band from O.band_indices(sr, n_fft, bands) and the mel bank from
    O.mel_filter_bank(sr, n_fft).  Everything else (bounds, forward_loss, the NAdam step, the best snapshot) is inherited."""

    def __init__(self, n_fft=O.N_FFT, hop=O.HOP, win_length=None, window="hann", sample_rate=O.SAMPLE_RATE, bands=BAND, **kw):
        super().__init__(**kw)
        self.n_fft, self.hop, self.sample_rate = n_fft, hop, sample_rate
        self.win = padded_window(window, n_fft if win_length is None else win_length, n_fft, self.dtype)
        self.band, self.nonband = O.band_indices(sample_rate, n_fft, bands)
        self.det.mel = torch.from_numpy(O.mel_filter_bank(sample_rate, n_fft)).to(self.dtype)

    def stft(self, x):
        return O.stft(x, self.n_fft, self.hop, self.win)

    def istft(self, X):
        return O.istft(X, self.n_fft, self.hop, self.win)

    def analyse(self, audio):
        x = audio / torch.amax(torch.abs(audio) + 1e-8, dim=-1, keepdim=True)
        S = self.stft(x)
        return torch.abs(S), torch.angle(S)

    def recompute_magnitude(self, mag_full, phase):
        y = self.istft(mag_full * torch.exp(1j * phase))
        y = y / torch.amax(torch.abs(y) + 1e-8, dim=-1, keepdim=True)
        y = y / torch.amax(torch.abs(y) + 1e-8, dim=-1, keepdim=True)
        return torch.abs(self.stft(y)), y

    def embed(self, audio, watermark, record=None):
        audio = torch.as_tensor(audio, dtype=self.dtype)
        target = torch.as_tensor(watermark, dtype=self.dtype)
        with torch.no_grad():
            mag0, phase = self.analyse(audio)
            c0 = mag0[:, self.band].clone()
            lo, hi = self.bounds(c0)
        c = c0.clone().requires_grad_(True)
        m, v = torch.zeros_like(c0), torch.zeros_like(c0)
        cg, cm, bc2 = O.nadam_schedule(self.num_iterations)
        best_loss = torch.full((audio.shape[0],), float("inf"), dtype=self.dtype)
        best_c = c0.clone()
        for it in range(self.num_iterations):
            c.grad = None
            loss, pred = self.forward_loss(c, mag0, phase, target)
            loss.sum().backward()
            with torch.no_grad():
                O.nadam_step(c.data, c.grad, m, v, cg[it], cm[it], bc2[it])
                c.data = torch.clamp(c.data, lo, hi)
                better = loss.detach() < best_loss
                best_loss = torch.where(better, loss.detach(), best_loss)
                best_c[better] = c.data[better]
            if record is not None:
                record(it, loss.detach().clone(), pred.detach().clone(), c.grad.detach().clone() if it == 0 else None,
                       c.data.clone(), lo, hi)
        with torch.no_grad():
            mag = mag0.clone()
            mag[:, self.band] = best_c
            y = self.istft(mag * torch.exp(1j * phase))
            y = y / torch.amax(torch.abs(y) + 1e-8, dim=-1, keepdim=True)
        return y, best_loss

    def detect_raw(self, audio):
        audio = torch.as_tensor(audio, dtype=self.dtype)
        with torch.no_grad():
            x = audio / torch.amax(torch.abs(audio) + 1e-8, dim=-1, keepdim=True)
            mag = torch.abs(self.stft(x)).clone()
            mag[:, self.nonband] = 0.0
            return self.det.forward(mag)

    def first_iteration(self, audio, watermark):
        """Loss [B], prediction [B, n_bits] and dL/dcoef [B, nband, T] of the first loop body, by autograd."""
        audio = torch.as_tensor(audio, dtype=self.dtype)
        with torch.no_grad():
            mag0, phase = self.analyse(audio)
        c = mag0[:, self.band].clone().requires_grad_(True)
        loss, pred = self.forward_loss(c, mag0, phase, torch.as_tensor(watermark, dtype=self.dtype))
        loss.sum().backward()
        return loss.detach(), pred.detach(), c.grad.detach()


def test_restatement_is_the_oracle_at_the_card_geometry():
    """GeneralLoop at 1024 / 256 / 1024, hann, 16 kHz, 500-4000 Hz against O.Embedder over 3 steps: per-step losses,
    predictions, the first gradient, the watermarked audio and the detector's values, bit for bit."""
    clips = np.stack([make_clip(s, 16000)[0] for s in (11, 12)])
    wm = np.stack([O.bits_to_bipolar(make_clip(s, 16000)[1]).astype(np.float32) for s in (11, 12)])
    a, b = [], []
    ya, la = O.Embedder(num_iterations=3).embed(clips, wm, record=lambda it, l, p, g: a.append((l, p, g)))
    yb, lb = GeneralLoop(num_iterations=3).embed(clips, wm, record=lambda it, l, p, g, *_: b.append((l, p, g)))
    assert len(a) == len(b) == 3
    for (l0, p0, g0), (l1, p1, g1) in zip(a, b):
        assert torch.equal(l0, l1) and torch.equal(p0, p1)
        assert (g0 is None) == (g1 is None) and (g0 is None or torch.equal(g0, g1))
    assert torch.equal(ya, yb) and torch.equal(la, lb)
    assert torch.equal(O.Embedder().detect_raw(ya.numpy()), GeneralLoop().detect_raw(yb.numpy()))


def test_padded_window_is_what_torch_stft_uses():
    """win_length < n_fft: the restatement's analysis against torch.stft with the short window."""
    x = torch.from_numpy(make_clip(5, 4000)[0])
    for name, fn in (("hann", torch.hann_window), ("hamming", torch.hamming_window)):
        ref = torch.stft(x, 512, 200, 400, fn(400), center=True, pad_mode="reflect", return_complex=True)
        mine = O.stft(x, 512, 200, padded_window(name, 400, 512))
        assert float((mine - ref).abs().max()) < 1e-4 * float(ref.abs().max())


GEOMS = [(n, h, w) for n, h, w, _, _, _ in TABLE] + [(512, 200, 400), (4096, 1024, 4096)]


def test_key_off_refuses_and_names_the_key():
    from aware_amd import runtime as rt
    from aware_amd.detection import AWAREDetector
    from aware_amd.embedding import AWAREEmbedder
    for n_fft, hop, win in GEOMS:
        if (n_fft, hop, win) == (1024, 256, 1024):
            continue
        for make in (lambda: AWAREEmbedder(frame_length=n_fft, hop_length=hop, win_length=win, verbose=False),
                     lambda: AWAREDetector(None, frame_length=n_fft, hop_length=hop, win_length=win),
                     lambda: rt.require_card_geometry("x", n_fft, hop, win)):
            with pytest.raises(NotImplementedError, match="model card") as exc:
                make()
            assert "general_geometry" in str(exc.value)
    emb = AWAREEmbedder(verbose=False, loss="push_extremes")
    assert emb.general_geometry is False and AWAREDetector(emb.detection_net).general_geometry is False


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("window", ["hann", "hamming"])
def test_key_on_constructs(geom, window):
    """With the key, every geometry runtime.check_geometry accepts constructs (no GPU is needed for that), the card's
    included; what check_geometry refuses is still refused."""
    from aware_amd.detection import AWAREDetector
    from aware_amd.embedding import AWAREEmbedder
    n_fft, hop, win = geom
    emb = AWAREEmbedder(frame_length=n_fft, hop_length=hop, win_length=win, window=window, general_geometry=True, verbose=False,
                        loss="push_extremes", detection_net_cfg={"n_fft": n_fft})
    det = AWAREDetector(emb.detection_net, frame_length=n_fft, hop_length=hop, win_length=win, window=window, general_geometry=True)
    assert emb.general_geometry and det.general_geometry
    assert emb.detection_net.mel_basis.shape == (128, n_fft // 2 + 1)


def test_key_on_still_checks_the_geometry():
    from aware_amd.embedding import AWAREEmbedder
    with pytest.raises(NotImplementedError, match="n_fft = 768"):
        AWAREEmbedder(frame_length=768, hop_length=192, win_length=768, general_geometry=True, detection_net_cfg={"n_fft": 768})
    with pytest.raises(ValueError, match="hop_length"):
        AWAREEmbedder(frame_length=512, hop_length=513, win_length=512, general_geometry=True, detection_net_cfg={"n_fft": 512})
    with pytest.raises(ValueError, match="window"):
        AWAREEmbedder(frame_length=512, hop_length=128, win_length=512, window="kaiser", general_geometry=True,
                      detection_net_cfg={"n_fft": 512})


def test_load_passes_the_key_through(tmp_path):
    from aware_amd.utils.models import load
    card = tmp_path / "card.yaml"
    card.write_text("frame_length: 2048\nhop_length: 512\nwin_length: 2048\ngeneral_geometry: true\n"
                    "detection_net_cfg: {sample_rate: 44100, n_fft: 2048}\nverbose: false\n")
    emb, det = load(str(card))
    assert emb.general_geometry and det.general_geometry and emb.frame_length == det.frame_length == 2048
    card.write_text("frame_length: 2048\nhop_length: 512\nwin_length: 2048\nverbose: false\n")
    assert load(str(card)) is None            # key absent: refused at construction, which load() reports as None


def test_mel_bank_has_to_follow_the_stft():
    from aware_amd.detection import AWAREDetector, AWAREDetectorNet
    from aware_amd.embedding import AWAREEmbedder
    with pytest.raises(ValueError, match="n_fft"):
        AWAREEmbedder(frame_length=512, hop_length=128, win_length=512, general_geometry=True, verbose=False, loss="push_extremes")
    with pytest.raises(ValueError, match="n_fft"):
        AWAREDetector(AWAREDetectorNet(), frame_length=512, hop_length=128, win_length=512, general_geometry=True)


def _embedder(n_fft, hop, win, window="hann", **kw):
    from aware_amd.embedding import AWAREEmbedder
    kw.setdefault("loss", "push_extremes")
    return AWAREEmbedder(frame_length=n_fft, hop_length=hop, win_length=win, window=window, general_geometry=True, verbose=False,
                         detection_net_cfg={"n_fft": n_fft}, **kw)


def test_clip_checks_name_the_clip():
    """Too short (n <= n_fft/2), NOLA, and a synthesis the loop's second STFT cannot pad: ValueError with the clip's index,
    from the host, before anything touches a device."""
    from aware_amd import runtime as rt
    from aware_amd.detection import AWAREDetector
    emb = _embedder(512, 128, 512)
    emb.check_clips([257, 4000])
    with pytest.raises(ValueError, match="clip 1 has 256 samples"):
        emb.check_clips([4000, 256])
    with pytest.raises(ValueError, match="clip 1 has 256 samples"):
        emb.embed_batch([np.zeros(4000, np.float32), np.zeros(256, np.float32)], 16000, np.ones((2, 20), np.float32))
    det = AWAREDetector(emb.detection_net, frame_length=512, hop_length=128, win_length=512, general_geometry=True)
    with pytest.raises(ValueError, match="clip 0 has 100 samples"):
        det.detect_batch([np.zeros(100, np.float32)], 16000)
    # a hann window at hop = n_fft is zero where neighbouring frames meet; a window shorter than the hop leaves gaps
    for n_fft, hop, win in ((512, 512, 512), (512, 200, 100)):
        assert not rt.nola_ok(n_fft, hop, win, "hann", 4000)
        with pytest.raises(ValueError, match="clip 0 .*NOLA"):
            _embedder(n_fft, hop, win).check_clips([4000, 700])
    assert rt.nola_ok(512, 200, 400, "hamming", 4000)
    # hop 100 at n_fft 1024: 599 samples give 6 frames (3 pooled) and a synthesis of 500 <= 512 samples
    with pytest.raises(ValueError, match="clip 0 .*synthesises to 500 samples"):
        _embedder(1024, 100, 1024).check_clips([599])
    _embedder(1024, 256, 1024).check_clips([513])        # 3 frames, one pooled frame: taken, as on the card route


def test_refusals_with_the_key_on():
    """What the general route does not serve raises NotImplementedError naming the feature and the key; nothing runs on the
    wrong period."""
    from aware_amd.detection import AWAREDetector
    from aware_amd.training import DetectorTrainer
    geom = dict(frame_length=512, hop_length=128, win_length=512, general_geometry=True)

    def refused(feature, fn):
        with pytest.raises(NotImplementedError, match=feature) as exc:
            fn()
        assert "general_geometry" in str(exc.value)

    refused("loop_attacks", lambda: _embedder(512, 128, 512, loop_attacks=[{"kind": "gaussian_noise", "snr_db": 10.0}]))
    refused("loop_attack_mixture", lambda: _embedder(512, 128, 512, loop_attack_mixture=[
        {"weight": 0.5, "chain": [{"kind": "gaussian_noise", "snr_db": 10.0}]}]))
    refused("push_extremes_l1", lambda: _embedder(512, 128, 512, loss="push_extremes_l1"))
    net = _embedder(512, 128, 512).detection_net
    refused("sync_search", lambda: AWAREDetector(net, sync_search=8, **geom))
    refused("speed_search", lambda: AWAREDetector(net, speed_search=5.0, **geom))
    det = AWAREDetector(net, **geom)
    clip = [np.zeros(16000, np.float32)]
    refused("sync_search", lambda: det.detect_batch(clip, 16000, sync_search=8))
    refused("speed_search", lambda: det.detect_batch(clip, 16000, speed_search=5.0))
    refused("scan", lambda: det.scan(clip, 16000))
    refused("DetectorTrainer", lambda: DetectorTrainer(det))


def test_stride_rule():
    """A general plan's band rows: the band's bins rounded up to a multiple of 64."""
    from aware_amd import runtime as rt
    from aware_amd.utils.audio import band_bins
    want = [256, 128, 64, 256, 256, 512, 960, 192]
    for (n_fft, _, _, sr, _, nband), stride in zip(TABLE, want):
        lo, hi = band_bins(sr, n_fft, BAND)
        assert hi - lo + 1 == nband == len(O.band_indices(sr, n_fft, BAND)[0])
        assert rt.general_band_stride(nband) == stride and stride % 64 == 0 and 0 <= stride - nband < 64
    lo, hi = band_bins(16000, 4096, (0, 8000))
    assert (lo, hi) == (0, 2048) and rt.general_band_stride(hi - lo + 1) == 2112


@pytest.mark.parametrize("geom", [(512, 128, 512, 16000, 16000), (2048, 512, 2048, 44100, 44100)])
def test_the_loop_works_at_other_geometries(geom):
    """The value claim on the CPU: four make_clip(s, n) clips, 400 steps, the card's detector seed, NAdam, 500-4000 Hz, 6 dB
    box.  Clean BER 0 % and mean |value| >= 0.15 (measured 0.258 and 0.257); the same clips unmarked read 0.017-0.021."""
    n_fft, hop, win, sr, n = geom
    clips = np.stack([make_clip(s, n)[0] for s in range(4)])
    bits = np.stack([make_clip(s, n)[1] for s in range(4)])
    loop = GeneralLoop(n_fft, hop, win, "hann", sr)
    y, _ = loop.embed(clips, O.bits_to_bipolar(bits).astype(np.float32))
    assert y.shape == (4, hop * (n // hop))
    vals = loop.detect_raw(y.numpy()).numpy()
    unmarked = float(np.abs(loop.detect_raw(clips).numpy()).mean())
    print(f"{n_fft} / {hop} / {win} at {sr} Hz: BER {O.ber_percent(O.decode_bits(vals), bits)} %, mean |value| "
          f"{float(np.abs(vals).mean()):.3f}, unmarked {unmarked:.3f}")
    assert O.ber_percent(O.decode_bits(vals), bits) == 0.0
    assert float(np.abs(vals).mean()) >= 0.15
