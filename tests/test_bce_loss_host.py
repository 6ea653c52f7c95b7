"""Host tests of the loss bce (F.binary_cross_entropy, embedding/losses.py, AWARE_LOSS_BCE) and of the unipolar configuration it
belongs to: pattern_mode bytes2bits, 0 / 1 targets, a detector that ends in sigmoid, threshold 0.5.

Also the torch restatements tests/test_gpu_bce_loss.py compares the device with: SigmoidDetector (the nets of this module,
in torch at a dtype), UnipolarLoop (the oracle's reference-shaped loop around it with a unipolar loss) and
first_iteration (loss, prediction and dL/dcoef of the first loop body).

The CPU convergence run (test_bce_converges_on_the_cpu): four make_clip clips of 1 s, the float32 restatement of E2E_NET,
400 NAdam steps, 6 dB box, the 24 bits of PAYLOAD as 0 / 1 targets, read at threshold 0.5.  Measured per clip (mean):
    bce            wrong bits 0 0 0 0, mean |v - 0.5| 0.0567 0.0568 0.0563 0.0568 (0.0566), SNR 14.61 14.32 14.39 14.62 dB (14.48)
    push_sigmoid   wrong bits 0 0 0 0, mean |v - 0.5| 0.0563 0.0566 0.0562 0.0570 (0.0565), SNR 14.59 14.33 14.49 14.56 dB (14.49)
bce reaches BER 0 on the CPU, and on this small net it is push_sigmoid's equal, not its better: the two rows differ by less
than their own spread over the clips (0.0005 and 0.0008 in mean |v - 0.5|, 0.30 and 0.26 dB in SNR).
"""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, make_clip
from oracle import aware_oracle as O

BLOCK = {"relu": torch.relu, "leaky_relu": lambda u: F.leaky_relu(u, 0.2), "gelu": F.gelu, "swish": F.silu}
FINAL = dict(BLOCK, tanh=torch.tanh, sigmoid=torch.sigmoid)

# the first-step network of the issue (output_length added per case) and the end-to-end network
NET = dict(final_activation="sigmoid", activation="gelu", norm_layer="instance", n_mels=128, num_blocks=2, n_filters=[128, 128])
E2E_NET = dict(NET, output_length=24)
PAYLOAD = b"\xA5\x3C\x0F"
STEPS = 400
# what the CPU run above measured, mean over the four clips: (wrong bits, mean |v - 0.5|, SNR dB)
CPU_RUN = {"bce": (0, 0.0566, 14.48), "push_sigmoid": (0, 0.0565, 14.49)}
# the largest spread (max - min) over the four clips in either row
SPREAD_DEV, SPREAD_SNR = 0.0008, 0.30


def make_net(**kw):
    from aware_amd.detection import AWAREDetectorNet
    return AWAREDetectorNet(**kw)


class SigmoidDetector:
    """AWAREDetectorNet.forward (multibit_detector_net.py:109-140, conv1d.py:38-42, BRH.py:16-27) in torch at `dtype`, for the
    nets of this module: mel -> InstanceNorm -> per-clip GlobalStandardize -> AvgPool1d(initial pool) -> blocks
    [Conv1d(kernel_size, stride, padding) + bias, norm, activation] -> BRH (time mean, even - odd) -> final activation.
    Restated here (as tests/test_detector_variants_host.py does for the 1x1 nets) so that this module stands alone."""

    def __init__(self, net, dtype=torch.float64):
        assert net.norm_layer in ("instance", "none")
        self.net = net
        self.mel = torch.from_numpy(net.mel_basis).to(dtype)
        self.ws = [torch.from_numpy(np.asarray(w)).to(dtype) for w in net.weights]
        self.bs = [torch.from_numpy(np.asarray(b)).to(dtype) for b in net.biases]
        self.act, self.fin = BLOCK[net.activation], FINAL[net.final_activation]

    @staticmethod
    def instance_norm(x, eps=1e-5):
        mu = x.mean(dim=-1, keepdim=True)
        return (x - mu) / torch.sqrt(x.var(dim=-1, unbiased=False, keepdim=True) + eps)

    def logits(self, mag):
        net = self.net
        x = self.instance_norm(torch.matmul(self.mel, mag))
        x = (x - x.mean(dim=(1, 2), keepdim=True)) / (x.std(dim=(1, 2), keepdim=True) + 1e-8)
        x = F.avg_pool1d(x, net.initial_pool_size, net.initial_pool_stride)
        for w, b in zip(self.ws, self.bs):
            z = F.conv1d(x, w if w.dim() == 3 else w[:, :, None], b, stride=net.stride, padding=net.padding)
            x = self.act(self.instance_norm(z) if net.norm_layer == "instance" else z)
        m = x.mean(dim=-1)
        return m[:, 0::2] - m[:, 1::2]

    def forward(self, mag):
        return self.fin(self.logits(mag))


def bce_per_clip(pred, target):
    """F.binary_cross_entropy with mean reduction, one value per clip."""
    return F.binary_cross_entropy(pred, target, reduction="none").mean(dim=-1)


class UnipolarLoop(O.Embedder):
    """The oracle's reference-shaped loop around `net` with the loss `loss` ("bce" or "push_sigmoid") on 0 / 1 targets, at
    the net's own n_fft with a full hann window and hop n_fft / 4 (the card geometry for the card's n_fft): analysis, the
    loop body and the detector's read are restated with that geometry; bounds, forward_loss, embed's NAdam step and best
    snapshot are the oracle's (embed itself synthesises at the card geometry only)."""

    def __init__(self, net, loss, dtype=torch.float32, bands=(500, 4000), **kw):
        super().__init__(loss="push_sigmoid", dtype=dtype, **kw)
        assert loss in ("bce", "push_sigmoid")
        if loss == "bce":
            self.loss = bce_per_clip
        self.det = SigmoidDetector(net, dtype)
        self.n_fft, self.hop = net.n_fft, net.n_fft // 4
        self.win = O.hann_window(self.n_fft, dtype)
        self.band, self.nonband = O.band_indices(net.sample_rate, self.n_fft, bands)

    def stft(self, x):
        return O.stft(x, self.n_fft, self.hop, self.win)

    def analyse(self, audio):
        x = audio / torch.amax(torch.abs(audio) + 1e-8, dim=-1, keepdim=True)
        S = self.stft(x)
        return torch.abs(S), torch.angle(S)

    def recompute_magnitude(self, mag_full, phase):
        y = O.istft(mag_full * torch.exp(1j * phase), self.n_fft, self.hop, self.win)
        y = y / torch.amax(torch.abs(y) + 1e-8, dim=-1, keepdim=True)
        y = y / torch.amax(torch.abs(y) + 1e-8, dim=-1, keepdim=True)
        return torch.abs(self.stft(y)), y

    def detect_raw(self, audio):
        audio = torch.as_tensor(audio, dtype=self.dtype)
        with torch.no_grad():
            x = audio / torch.amax(torch.abs(audio) + 1e-8, dim=-1, keepdim=True)
            mag = torch.abs(self.stft(x)).clone()
            mag[:, self.nonband] = 0.0
            return self.det.forward(mag)


def first_iteration(emb, clip, target):
    """Loss, prediction [n_bits] and dL/dcoef [nband, T] of the loop's first body (multibit_embedder.py:95-111), by autograd."""
    a = torch.from_numpy(clip).to(emb.dtype)[None]
    mag0, phase = emb.analyse(a)
    c0 = mag0[:, emb.band].clone().requires_grad_(True)
    l, p = emb.forward_loss(c0, mag0, phase, torch.from_numpy(target).to(emb.dtype)[None])
    l.sum().backward()
    return float(l.detach()), p[0].detach().numpy(), c0.grad[0].numpy()


def payload_bits():
    from aware_amd.utils.watermark import PatternEncoder
    return np.asarray(PatternEncoder(mode="bytes2bits")(PAYLOAD), dtype=np.int32)


def snr_db(host, marked):
    """SNR of the loop's output against the peak-normalised host clip over their common length (metrics/audio.py:68-89)."""
    n = min(len(host), len(marked))
    x = host[:n] / np.max(np.abs(host[:n]) + 1e-8)
    return float(10 * np.log10(np.sum(x ** 2) / np.sum((marked[:n] - x) ** 2)))


# ---- the registry ------------------------------------------------------------------------------------------------------
def test_registry_refuses_and_accepts():
    from aware_amd.embedding.losses import BinaryCrossEntropyLoss, get_loss_fn
    with pytest.raises(NotImplementedError, match="sigmoid"):
        get_loss_fn("bce")
    fn = get_loss_fn("bce", final_activation="sigmoid")
    assert isinstance(fn, BinaryCrossEntropyLoss) and fn.kernel_id == 8 and fn.name == "bce"
    for other in ("tanh", "relu", "gelu"):
        with pytest.raises(NotImplementedError, match="final_activation"):
            get_loss_fn("bce", final_activation=other)
    # the keyword changes no other loss
    assert get_loss_fn("push_sigmoid", final_activation="tanh").kernel_id == 4
    with pytest.raises(ValueError, match="Unknown loss type"):
        get_loss_fn("push", final_activation="sigmoid")
    from aware_amd import runtime as rt
    assert rt.LOSS_KINDS["bce"] == 8 and sorted(rt.LOSS_KINDS.values()) == [0, 1, 2, 3, 4, 5, 6, 8]


def test_forward_is_torch_bce_with_its_clamp():
    from aware_amd.embedding.losses import get_loss_fn
    fn = get_loss_fn("bce", final_activation="sigmoid")
    rng = np.random.default_rng(3)
    p = torch.from_numpy(rng.uniform(0, 1, (4, 20)).astype(np.float32))
    t = torch.from_numpy(rng.integers(0, 2, (4, 20)).astype(np.float32))
    assert torch.equal(fn.forward(p, t), F.binary_cross_entropy(p, t))
    edge = torch.tensor([0.0, 1.0, 1e-45, 1.0 - 2.0 ** -24], dtype=torch.float32)
    assert float(edge[3]) < 1.0
    for tv in (0.0, 1.0):
        tt = torch.full_like(edge, tv)
        assert torch.equal(fn.forward(edge, tt), F.binary_cross_entropy(edge, tt))
        each = F.binary_cross_entropy(edge, tt, reduction="none")
        assert torch.isfinite(each).all()
        assert float(each[0]) == (100.0 if tv else 0.0) and float(each[1]) == (0.0 if tv else 100.0)     # the clamp at -100


def test_the_formulas_the_kernel_uses_are_torch_autograd():
    """csrc/common.hpp::loss_term_bce: l = (t - 1) max(log1p(-p), -100) - t max(log p, -100), dl/dp = (p - t) / max(p (1 - p),
    1e-12), both times 1 / n_bits; and through a sigmoid the gradient at a saturated p is exactly 0."""
    p = torch.tensor([0.0, 1.0, 1.0 - 2.0 ** -24, 1e-10, 0.3, 0.5, 0.9999], dtype=torch.float32)
    for tv in (0.0, 1.0):
        t = torch.full_like(p, tv)
        q = p.clone().requires_grad_(True)
        l = F.binary_cross_entropy(q, t, reduction="none")
        l.sum().backward()
        mine = (t - 1) * torch.clamp(torch.log1p(-p), min=-100) - t * torch.clamp(torch.log(p), min=-100)
        assert torch.equal(mine, l.detach())
        assert torch.equal((p - t) / torch.clamp((1 - p) * p, min=1e-12), q.grad)
        assert torch.isfinite(q.grad).all()
    x = torch.tensor([-200.0, -120.0, 120.0, 200.0], dtype=torch.float32, requires_grad=True)
    s = torch.sigmoid(x)
    assert s.detach().tolist() == [0.0, 0.0, 1.0, 1.0]
    F.binary_cross_entropy(s, torch.tensor([1.0, 0.0, 0.0, 1.0])).backward()
    assert x.grad.tolist() == [0.0, 0.0, 0.0, 0.0]


def test_header_constants():
    text = open(os.path.join(ROOT, "include", "aware_hip.h")).read()
    kinds = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define AWARE_LOSS_(\w+) (\d+)", text)}
    assert kinds["BCE"] == 8 and kinds["EXTERNAL"] == 7
    assert sorted(kinds.values()) == list(range(9))


# ---- the embedder ------------------------------------------------------------------------------------------------------
def unipolar_embedder(**kw):
    from aware_amd.embedding import AWAREEmbedder
    return AWAREEmbedder(pattern_mode="bytes2bits", loss="bce", verbose=False, detection_net_cfg=dict(E2E_NET), **kw)


def test_embedder_refuses_tanh_and_takes_sigmoid():
    from aware_amd.embedding import AWAREEmbedder
    with pytest.raises(NotImplementedError, match="final_activation"):
        AWAREEmbedder(loss="bce", verbose=False)                                    # the card's network with loss: bce
    with pytest.raises(NotImplementedError, match="final_activation"):
        AWAREEmbedder(loss="bce", verbose=False, detection_net_cfg={"final_activation": "relu"})
    emb = unipolar_embedder()                    # construction needs no device library
    assert emb.loss.name == "bce" and emb.loss.kernel_id == 8 and emb.detection_net.final_activation == "sigmoid"
    assert AWAREEmbedder(loss="bce", verbose=False, detection_net_cfg={"final_activation": "Sigmoid"}).loss.name == "bce"


def test_load_with_a_unipolar_card(tmp_path):
    import yaml
    from aware_amd.utils.models import load
    from aware_amd.utils.models.load_model import _CARD
    card = yaml.safe_load(open(_CARD))
    card.update(pattern_mode="bytes2bits", loss="bce", threshold=0.5)
    card["detection_net_cfg"] = dict(card.get("detection_net_cfg") or {}, final_activation="sigmoid", output_length=24)
    path = tmp_path / "unipolar.yaml"
    path.write_text(yaml.safe_dump(card))
    emb, det = load(str(path))
    assert emb.loss.name == "bce" and emb.pattern_mode == "bytes2bits"
    assert det.threshold == 0.5 and det.pattern_mode == "bytes2bits" and det.detection_net is emb.detection_net
    card["detection_net_cfg"]["final_activation"] = "tanh"
    path.write_text(yaml.safe_dump(card))
    assert load(str(path)) is None               # the card's network with loss: bce: refused when the embedder is built


@pytest.mark.parametrize("bad", [-1.0, 2.0, float("nan")])
def test_targets_outside_the_unit_interval_raise(bad):
    emb = unipolar_embedder()
    clip = make_clip(0, 16000)[0]
    wm = payload_bits().astype(np.float32)
    wm[5] = bad
    with pytest.raises(ValueError, match="between 0 and 1"):
        emb.embed_batch([clip], 16000, wm[None])
    with pytest.raises(ValueError, match="between 0 and 1"):
        emb.embed(clip, 16000, wm)
    emb.check_targets(payload_bits()[None])                       # 0 / 1: taken
    emb.check_targets(np.full((1, 24), 0.5, np.float32))          # torch takes soft targets too
    from aware_amd.embedding import AWAREEmbedder
    other = AWAREEmbedder(loss="push_sigmoid", verbose=False, detection_net_cfg=dict(E2E_NET))
    other.check_targets(wm[None])                                  # no other loss has a rule


# ---- convergence on the CPU --------------------------------------------------------------------------------------------
def cpu_run(loss):
    """(wrong bits, mean |v - 0.5|, SNR dB) per clip of the float32 restatement's 400-step embed of four 1 s clips."""
    net = make_net(**E2E_NET)
    clips = np.stack([make_clip(s, 16000)[0] for s in range(4)])
    bits = payload_bits()
    emb = UnipolarLoop(net, loss, num_iterations=STEPS)
    y, _ = emb.embed(clips, np.tile(bits.astype(np.float32), (4, 1)))
    vals = emb.detect_raw(y.numpy()).numpy()
    wrong = ((vals > 0.5).astype(np.int32) != bits).sum(axis=1)
    return wrong, np.abs(vals - 0.5).mean(axis=1), np.array([snr_db(clips[i], y[i].numpy()) for i in range(4)])


def test_bce_converges_on_the_cpu():
    """What the restatement itself delivers (module docstring): no wrong bit on any clip with either loss, and every clip's
    mean |v - 0.5| and SNR within two spreads (the largest max - min over the four clips in either row) of the recorded mean
    of its row -- so also: the two losses within four spreads of each other."""
    rows = {loss: cpu_run(loss) for loss in ("bce", "push_sigmoid")}
    for loss, (wrong, dev, snr) in rows.items():
        print(f"{loss}: wrong bits {wrong.tolist()}, mean |v - 0.5| {np.round(dev, 4).tolist()} (mean {dev.mean():.4f}), "
              f"SNR {np.round(snr, 2).tolist()} dB (mean {snr.mean():.2f})")
    for loss, (wrong, dev, snr) in rows.items():
        assert wrong.tolist() == [CPU_RUN[loss][0]] * 4, (loss, wrong)
        assert np.abs(dev - CPU_RUN[loss][1]).max() < 2 * SPREAD_DEV, (loss, dev)
        assert np.abs(snr - CPU_RUN[loss][2]).max() < 2 * SPREAD_SNR, (loss, snr)
