"""CPU tests of detector sizes other than the model card's (detection_net_cfg n_mels, num_blocks, n_filters): the float64
restatement the GPU tests hold the kernels to (checked against the reference's own outputs in tests/golden/detector_sizes.npz,
written by tools/make_golden_sizes.py), the seeded weights, the storage rule's host mirror, the caps, the training refusal and
load() of an edited card."""
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from test_detector_variants_host import VariantDetector, fixture_magnitudes, push_extremes_sum

FIXTURE = os.path.join(GOLDEN, "detector_sizes.npz")
CARD = dict(n_mels=128, num_blocks=3, n_filters=[512, 1024, 1024], output_length=20, activation="leaky_relu",
            norm_layer="instance", final_activation="tanh")
# tools/make_golden_sizes.py CONFIGS (edits of the card's detection_net_cfg)
CONFIGS = {
    "m40": dict(n_mels=40),
    "m64": dict(n_mels=64),
    "m80_2blk": dict(n_mels=80, num_blocks=2, n_filters=[256, 256]),
    "m200": dict(n_mels=200),
    "m13_odd": dict(n_mels=13, num_blocks=2, n_filters=[30, 61], output_length=7),
    "f_odd": dict(n_filters=[250, 500, 750]),
    "deep10": dict(num_blocks=10, n_filters=[256] * 10),
    "blk0": dict(n_mels=96, num_blocks=0, n_filters=[]),
    "m64_gelu_batch_sigmoid": dict(n_mels=64, num_blocks=2, n_filters=[100, 202], activation="gelu", norm_layer="batch",
                                   final_activation="sigmoid"),
    "m64_L64": dict(n_mels=64, output_length=64),
}
TRAJ = {"m64": dict(n_mels=64, num_blocks=3, n_filters=[250, 500, 750]), "m80": dict(n_mels=80, num_blocks=8, n_filters=[256] * 8)}


def config(name):
    return dict(CARD, **CONFIGS[name])


def oracle_net(cfg):
    """The network of `cfg` built from the oracle's helpers (mel_filter_bank(n_mels=), detector_weights(n_mels=, n_filters=)),
    in the attribute shape VariantDetector reads; BatchNorm as a fresh net in eval mode."""
    from oracle import aware_oracle as O
    ws, bs = O.detector_weights(n_mels=cfg["n_mels"], n_filters=tuple(cfg["n_filters"]), output_length=cfg["output_length"])
    ws = [w.numpy() for w in ws]
    bn = None
    if cfg["norm_layer"] == "batch":
        bn = [{"weight": np.ones(w.shape[0]), "bias": np.zeros(w.shape[0]), "running_mean": np.zeros(w.shape[0]),
               "running_var": np.ones(w.shape[0]), "eps": 1e-5} for w in ws]
    return types.SimpleNamespace(mel_basis=O.mel_filter_bank(n_mels=cfg["n_mels"]), weights=ws, biases=[b.numpy() for b in bs],
                                 batch_norm=bn, activation=cfg["activation"], norm_layer=cfg["norm_layer"],
                                 final_activation=cfg["final_activation"])


def test_fixture_covers_every_config():
    f = np.load(FIXTURE)
    assert [str(v) for v in f["configs"]] == list(CONFIGS)
    for name in CONFIGS:
        L = config(name)["output_length"]
        assert f[f"net/{name}/pred"].shape == (2, L, 1)
        assert f[f"net/{name}/grad"].shape == (2, 225, 8)
        assert f[f"net/{name}/target"].shape == (2, L, 1)
    for name in TRAJ:
        assert f[f"traj/{name}/losses"].shape == (400,)
        np.testing.assert_array_equal(f[f"traj/{name}/det_bits"], f[f"traj/{name}/bits"])   # the reference recovers its bits
    assert os.path.getsize(FIXTURE) < 1 << 20


@pytest.mark.parametrize("name", list(CONFIGS))
def test_float64_restatement_matches_the_reference(name):
    f = np.load(FIXTURE)
    det = VariantDetector(oracle_net(config(name)))
    mag = torch.from_numpy(fixture_magnitudes()).double().requires_grad_(True)
    pred = det.forward(mag)
    push_extremes_sum(pred, torch.from_numpy(f[f"net/{name}/target"]).double()).backward()
    np.testing.assert_allclose(pred.detach().numpy(), f[f"net/{name}/pred"][..., 0], atol=2e-6)
    g, ref = mag.grad.numpy()[:, 32:257, ::int(f["grad_step"])], f[f"net/{name}/grad"]
    for b in range(g.shape[0]):
        rel = np.linalg.norm(g[b] - ref[b]) / np.linalg.norm(ref[b])
        assert rel < 1e-4, (name, b, rel)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_network_channels_and_weights(name):
    from aware_amd.detection import AWAREDetectorNet
    cfg = config(name)
    net = AWAREDetectorNet(**cfg)
    assert net.channels == [cfg["n_mels"]] + cfg["n_filters"] + [2 * cfg["output_length"]]
    ref = oracle_net(cfg)
    np.testing.assert_array_equal(net.mel_basis, ref.mel_basis)
    assert len(net.weights) == cfg["num_blocks"] + 1
    for a, b in zip(net.weights, ref.weights):             # the reference's seeded xavier draws
        np.testing.assert_array_equal(a, b)


def test_storage_rule_mirror():
    from aware_amd import runtime as rt
    # every network the library accepted before maps to itself
    assert rt.stored_channels([128, 512, 1024, 1024, 40]) == [128, 512, 1024, 1024, 40]
    assert rt.stored_channels([128, 100, 204, 8]) == [128, 100, 204, 8]
    assert rt.stored_channels([128, 256, 64]) == [128, 256, 64]
    # the mel bank: a multiple of 4 as is (128 -> 128), else up to a multiple of 4 (<= 64) or 128
    assert [rt.stored_channels([m, 256, 40])[0] for m in (128, 40, 64, 80, 96, 200, 13, 1, 63, 65, 125, 510)] == \
        [128, 40, 64, 80, 96, 200, 16, 4, 64, 128, 128, 512]
    # hidden widths: the same rule; the last block as before (even 2 .. 1024: a multiple of 4 up to 64, of 128 above)
    assert rt.stored_channels([13, 30, 61, 14]) == [16, 32, 64, 16]
    assert rt.stored_channels([128, 250, 500, 750, 40]) == [128, 256, 500, 768, 40]
    assert rt.stored_channels([128, 202, 100, 128]) == [128, 256, 100, 128]
    assert rt.stored_channels([96, 1000]) == [96, 1024]
    assert rt.stored_channels([96, 66]) == [96, 128]
    assert rt.stored_channels([64, 4095, 40]) == [64, 4096, 40]
    for ch in ([40, 1, 2], [512, 4096, 1024], [7, 9, 11, 13, 22]):
        st = rt.stored_channels(ch)
        assert all(s >= c and s % 4 == 0 for s, c in zip(st, ch))


def test_caps():
    from aware_amd.detection import AWAREDetectorNet
    AWAREDetectorNet(n_mels=512, num_blocks=1, n_filters=[4096])
    AWAREDetectorNet(n_mels=1, num_blocks=0, n_filters=[])
    AWAREDetectorNet(num_blocks=32, n_filters=[8] * 32)
    with pytest.raises(NotImplementedError, match="512"):
        AWAREDetectorNet(n_mels=513)
    with pytest.raises(NotImplementedError, match="4096"):
        AWAREDetectorNet(num_blocks=1, n_filters=[4097])
    with pytest.raises(NotImplementedError, match="32"):
        AWAREDetectorNet(num_blocks=33, n_filters=[8] * 33)
    for kw in (dict(n_mels=0), dict(num_blocks=1, n_filters=[0]), dict(num_blocks=-1, n_filters=[])):
        with pytest.raises((ValueError, AssertionError)):
            AWAREDetectorNet(**kw)
    with pytest.raises(ValueError):
        AWAREDetectorNet(n_mels=0)
    with pytest.raises(AssertionError):                  # the reference's own assertion
        AWAREDetectorNet(num_blocks=2, n_filters=[8])


def test_training_refusal():
    from aware_amd import runtime as rt
    assert rt.training_refusal([128, 512, 1024, 1024, 40]) is None
    assert rt.training_refusal([128, 100, 40]) is None
    assert rt.training_refusal([128] + [256] * 6 + [40]) is None
    assert "n_mels" in rt.training_refusal([64, 512, 1024, 1024, 40])
    assert "num_blocks" in rt.training_refusal([128] + [256] * 7 + [40])
    assert "n_filters" in rt.training_refusal([128, 250, 500, 750, 40])


def test_detector_trainer_refuses_the_new_sizes():
    from aware_amd.detection import AWAREDetectorNet
    from aware_amd.training import DetectorTrainer
    for kw in (dict(n_mels=64), dict(n_filters=[250, 500, 750]), dict(num_blocks=7, n_filters=[64] * 7)):
        det = types.SimpleNamespace(detection_net=AWAREDetectorNet(**kw))
        with pytest.raises(NotImplementedError, match="DetectorTrainer"):
            DetectorTrainer(det)


def test_load_with_an_edited_card(tmp_path):
    import yaml
    from aware_amd.utils.models import load
    card = yaml.safe_load(open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")))
    card["detection_net_cfg"] = dict(card["detection_net_cfg"], n_mels=64, num_blocks=2, n_filters=[250, 500])
    path = tmp_path / "config.yaml"
    path.write_text(yaml.safe_dump(card))
    out = load(str(path))
    assert out is not None
    emb, det = out
    assert det.detection_net is emb.detection_net
    assert emb.detection_net.channels == [64, 250, 500, 40]
    assert emb.detection_net.mel_basis.shape == (64, 513)


def test_header_declares_version_350():
    text = open(os.path.join(ROOT, "include", "aware_hip.h")).read()
    assert re.search(r"350: detector sizes", text)
    src = open(os.path.join(ROOT, "aware_amd", "csrc", "capi.hip")).read()
    assert 'aware_version(void) { return 350; }' in src
