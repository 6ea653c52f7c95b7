"""CPU tests of payload lengths other than the model card's 20 bits (watermark_length / detection_net_cfg.output_length 1..512):
the float64 restatement the GPU tests hold the kernels to (checked against the reference's own outputs in
tests/golden/payload_lengths.npz, written by tools/make_golden_payload.py), the network's shapes, the refusal above 512 bits,
load() of an edited card and the multi-byte pattern encoder."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from test_detector_variants_host import fixture_magnitudes, push_extremes_sum

FIXTURE = os.path.join(GOLDEN, "payload_lengths.npz")
LENGTHS = (1, 21, 33, 64, 128, 512)


class PayloadDetector:
    """The card's detector (multibit_detector_net.py:109-140) with an L-bit read-out, in float64, built from the oracle's
    helpers: mel_filter_bank() and detector_weights(output_length=L).  Batched per clip as oracle.Detector."""

    def __init__(self, L, dtype=torch.float64):
        from oracle import aware_oracle as O
        self.mel = torch.from_numpy(O.mel_filter_bank()).to(dtype)
        ws, bs = O.detector_weights(output_length=L)
        self.ws = [w.to(dtype) for w in ws]
        self.bs = [b.to(dtype) for b in bs]
        self.O = O

    def forward(self, mag):
        x = torch.matmul(self.mel, mag)
        x = self.O.Detector.instance_norm(x)
        x = (x - x.mean(dim=(1, 2), keepdim=True)) / (x.std(dim=(1, 2), keepdim=True) + 1e-8)
        x = torch.nn.functional.avg_pool1d(x, 2, 2)
        for w, b in zip(self.ws, self.bs):
            x = torch.nn.functional.leaky_relu(self.O.Detector.instance_norm(torch.matmul(w, x) + b[:, None]), 0.2)
        m = x.mean(dim=-1)
        return torch.tanh(m[:, 0::2] - m[:, 1::2])


def test_fixture_covers_every_length():
    f = np.load(FIXTURE)
    assert tuple(int(v) for v in f["lengths"]) == LENGTHS
    for L in LENGTHS:
        assert f[f"net/L{L}/pred"].shape == (2, L, 1)
        assert f[f"net/L{L}/grad"].shape == (2, 225, 8)
    assert f["traj/L64/losses"].shape == (400,)
    assert f["traj/L64/bits"].shape == (64,)
    np.testing.assert_array_equal(f["traj/L64/det_bits"], f["traj/L64/bits"])   # the reference recovers its 64 bits
    assert os.path.getsize(FIXTURE) < 1 << 20


@pytest.mark.parametrize("L", LENGTHS)
def test_float64_restatement_matches_the_reference(L):
    f = np.load(FIXTURE)
    det = PayloadDetector(L)
    mag = torch.from_numpy(fixture_magnitudes()).double().requires_grad_(True)
    pred = det.forward(mag)
    push_extremes_sum(pred, torch.from_numpy(f[f"net/L{L}/target"]).double()).backward()
    np.testing.assert_allclose(pred.detach().numpy(), f[f"net/L{L}/pred"][..., 0], atol=2e-6)
    g, ref = mag.grad.numpy()[:, 32:257, ::int(f["grad_step"])], f[f"net/L{L}/grad"]
    for b in range(g.shape[0]):
        rel = np.linalg.norm(g[b] - ref[b]) / np.linalg.norm(ref[b])
        assert rel < 1e-4, (L, b, rel)


@pytest.mark.parametrize("L", LENGTHS)
def test_network_shapes_and_weights(L):
    from aware_amd.detection import AWAREDetectorNet
    from oracle import aware_oracle as O
    net = AWAREDetectorNet(output_length=L)
    assert net.output_length == L
    assert net.channels == [128, 512, 1024, 1024, 2 * L]
    assert [w.shape for w in net.weights][-1] == (2 * L, 1024)
    assert net.biases[-1].shape == (2 * L,)
    n = sum(w.size for w in net.weights) + sum(b.size for b in net.biases)
    assert n == 128 * 512 + 512 + 512 * 1024 + 1024 + 1024 * 1024 + 1024 + 1024 * 2 * L + 2 * L
    ws, _ = O.detector_weights(output_length=L)
    for a, b in zip(net.weights, ws):                  # the same seeded xavier draws as the reference
        np.testing.assert_array_equal(a, b.numpy())


def test_lengths_above_512_are_refused():
    from aware_amd.detection import AWAREDetectorNet
    AWAREDetectorNet(output_length=512)
    with pytest.raises(NotImplementedError, match="512"):
        AWAREDetectorNet(output_length=513)
    with pytest.raises(NotImplementedError, match="512"):
        AWAREDetectorNet(output_length=4096)


def test_load_with_an_edited_card(tmp_path):
    import yaml
    from aware_amd.utils.models import load
    card = yaml.safe_load(open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")))
    card["watermark_length"] = 64
    card["detection_net_cfg"] = dict(card["detection_net_cfg"], output_length=64)
    path = tmp_path / "config.yaml"
    path.write_text(yaml.safe_dump(card))
    out = load(str(path))
    assert out is not None
    emb, det = out
    assert det.detection_net is emb.detection_net
    assert emb.detection_net.output_length == 64
    assert emb.detection_net.channels[-1] == 128


def test_bytes2bipolar_multi_byte_payload():
    from aware_amd.utils.watermark.codec import PatternEncoder
    payload = bytes([0x00, 0xFF, 0x5A, 0x01, 0x80, 0x7E, 0xC3, 0x10])
    v = np.asarray(PatternEncoder("bytes2bipolar")(payload))
    assert v.size == 64
    bits = np.unpackbits(np.frombuffer(payload, np.uint8))
    np.testing.assert_array_equal(v.reshape(-1), 2 * bits.astype(np.int64) - 1)
