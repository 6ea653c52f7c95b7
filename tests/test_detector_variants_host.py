"""CPU tests of the detector's architecture variants (detection_net_cfg: activation, norm_layer, final_activation):
construction semantics of the reference, seed-identical weights, load() of an edited card, the refusals that remain, the
C ABI's new symbols, and the float64 restatement the GPU tests hold the kernels to (checked here against the reference's
own outputs in tests/golden/detector_variants.npz, written by tools/make_golden_variants.py)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

FIXTURE = os.path.join(GOLDEN, "detector_variants.npz")
BLOCK = {"relu": torch.relu, "leaky_relu": lambda u: torch.nn.functional.leaky_relu(u, 0.2),
         "gelu": torch.nn.functional.gelu, "swish": torch.nn.functional.silu}
FINAL = dict(BLOCK, tanh=torch.tanh, sigmoid=torch.sigmoid)


def fixture_magnitudes(seed=77, shape=(2, 513, 63)):
    """tools/make_golden_variants.py magnitudes(): |complex Gaussian| in bins 32..256, zero elsewhere."""
    rng = np.random.default_rng(seed)
    m = np.zeros(shape, np.float32)
    z = rng.standard_normal((shape[0], 225, shape[2], 2))
    m[:, 32:257, :] = (0.3 * np.hypot(z[..., 0], z[..., 1])).astype(np.float32)
    return m


def variant_keys():
    f = np.load(FIXTURE)
    return sorted({k.split("/")[1] for k in f.files if k.startswith("net/")})


def split_key(key):
    """'leaky_relu_instance_tanh' -> ('leaky_relu', 'instance', 'tanh')."""
    m = re.fullmatch(r"(relu|leaky_relu|gelu|swish)_(instance|batch|none)_(\w+)", key)
    return m.group(1), m.group(2), m.group(3)


class VariantDetector:
    """AWAREDetectorNet.forward (multibit_detector_net.py:109-140, conv1d.py:38-42, BRH.py:16-27) for any architecture, in
    torch at `dtype`, batched per clip as oracle.Detector: mel -> InstanceNorm -> per-clip GlobalStandardize -> AvgPool(2) ->
    blocks [conv + bias, norm, activation] -> BRH (time mean, even - odd) -> final activation.  BatchNorm in eval mode."""

    def __init__(self, net, dtype=torch.float64):
        self.net = net
        self.mel = torch.from_numpy(net.mel_basis).to(dtype)
        self.ws = [torch.from_numpy(w).to(dtype) for w in net.weights]
        self.bs = [torch.from_numpy(b).to(dtype) for b in net.biases]
        self.bn = None
        if net.batch_norm is not None:
            self.bn = [{k: (torch.as_tensor(v).to(dtype) if k != "eps" else v) for k, v in p.items()} for p in net.batch_norm]
        self.act, self.fin = BLOCK[net.activation], FINAL[net.final_activation]

    @staticmethod
    def instance_norm(x, eps=1e-5):
        mu = x.mean(dim=-1, keepdim=True)
        return (x - mu) / torch.sqrt(x.var(dim=-1, unbiased=False, keepdim=True) + eps)

    def pre_activations(self, mag):
        """The input of every block activation ([B, C, T/2] each) and of the final activation ([B, 20])."""
        x = self.instance_norm(torch.matmul(self.mel, mag))
        x = (x - x.mean(dim=(1, 2), keepdim=True)) / (x.std(dim=(1, 2), keepdim=True) + 1e-8)
        x = torch.nn.functional.avg_pool1d(x, 2, 2)
        us = []
        for l, (w, b) in enumerate(zip(self.ws, self.bs)):
            z = torch.matmul(w, x) + b[:, None]
            if self.net.norm_layer == "instance":
                u = self.instance_norm(z)
            elif self.net.norm_layer == "batch":
                p = self.bn[l]
                u = (z - p["running_mean"][:, None]) / torch.sqrt(p["running_var"][:, None] + p["eps"]) * p["weight"][:, None] + \
                    p["bias"][:, None]
            else:
                u = z
            us.append(u)
            x = self.act(u)
        m = x.mean(dim=-1)
        us.append(m[:, 0::2] - m[:, 1::2])
        return us

    def forward(self, mag):
        return self.fin(self.pre_activations(mag)[-1])

    def kink_distance(self, mag):
        """Per clip, the smallest |u| over the arguments of ReLU / LeakyReLU (blocks and read-out; inf without such a kink):
        where some |u| is within rounding of 0 the sign, and with it a finite part of the gradient, is decided by rounding."""
        with torch.no_grad():
            us = self.pre_activations(mag)
        d = torch.full((mag.shape[0],), float("inf"), dtype=torch.float64)
        kinks = ("relu", "leaky_relu")
        for i, u in enumerate(us):
            name = self.net.final_activation if i == len(us) - 1 else self.net.activation
            if name in kinks:
                d = torch.minimum(d, u.abs().reshape(u.shape[0], -1).min(dim=1).values.double())
        return d.numpy()


def push_extremes_sum(pred, target):
    """Sum over clips of PushToExtremesLoss (losses.py:38-42) per clip: pred, target [B, 20(, 1)]."""
    p, t = pred.reshape(pred.shape[0], -1), target.reshape(target.shape[0], -1)
    return (((p - t) ** 2).mean(dim=1) - 0.1 * p.abs().mean(dim=1)).sum()


def test_construction_semantics_match_the_reference():
    from aware_amd.detection import AWAREDetectorNet
    from aware_amd.detection.multibit_detector_net import block_activation
    # Conv1dBlock._get_activation: case-insensitive, anything unknown silently becomes ReLU
    for given, built in (("ReLU", "relu"), ("LEAKY_RELU", "leaky_relu"), ("Gelu", "gelu"), ("swish", "swish"),
                         ("tanh", "relu"), ("sigmoid", "relu"), ("mish", "relu"), ("", "relu")):
        assert block_activation(given) == built
        assert AWAREDetectorNet(activation=given).activation == built
    # Conv1dBlock._get_norm_layer and AWAREDetectorNet._get_activation raise ValueError
    with pytest.raises(ValueError, match="Invalid norm layer"):
        AWAREDetectorNet(norm_layer="layer")
    with pytest.raises(ValueError, match="Invalid activation"):
        AWAREDetectorNet(final_activation="softmax")
    # the reference builds the blocks (norm check) before the head (final activation check)
    with pytest.raises(ValueError, match="Invalid norm layer"):
        AWAREDetectorNet(norm_layer="group", final_activation="softmax")
    for fin in ("RELU", "leaky_relu", "gelu", "Swish", "tanh", "SIGMOID"):
        assert AWAREDetectorNet(final_activation=fin).final_activation == fin.lower()
    for norm in ("Instance", "BATCH", "none"):
        assert AWAREDetectorNet(norm_layer=norm).norm_layer == norm.lower()
    card = AWAREDetectorNet()
    assert card.is_card_arch and (card.activation, card.norm_layer, card.final_activation) == ("leaky_relu", "instance", "tanh")
    assert not AWAREDetectorNet(final_activation="sigmoid").is_card_arch
    info = AWAREDetectorNet(activation="gelu", norm_layer="batch", final_activation="sigmoid").get_model_info()
    assert (info["activation"], info["norm_layer"], info["final_activation"]) == ("gelu", "batch", "sigmoid")
    # BatchNorm1d adds weight + bias per block to the reference's parameters(); InstanceNorm1d (affine=False) adds none
    assert info["total_parameters"] == 1681960 + 2 * (512 + 1024 + 1024 + 40)
    assert AWAREDetectorNet(norm_layer="none").get_model_info()["total_parameters"] == 1681960


def test_weights_do_not_depend_on_the_architecture():
    """BatchNorm has no Conv / Linear weight, so the xavier draws of the seed are the same for every variant."""
    from aware_amd.detection import AWAREDetectorNet
    card = AWAREDetectorNet()
    g = np.load(os.path.join(GOLDEN, "weights.npz"))
    for act in ("relu", "leaky_relu", "gelu", "swish", "unknown"):
        for norm in ("instance", "batch", "none"):
            for fin in ("relu", "tanh", "sigmoid"):
                net = AWAREDetectorNet(activation=act, norm_layer=norm, final_activation=fin)
                for a, b in zip(net.weights + net.biases, card.weights + card.biases):
                    np.testing.assert_array_equal(a, b)
                for i, w in enumerate(net.weights):
                    np.testing.assert_array_equal(w[:4, :8], g[f"w{i}_corner"])


def test_batch_norm_folds_to_the_eval_mode_affine_map():
    from aware_amd.detection import AWAREDetectorNet
    net = AWAREDetectorNet(norm_layer="batch")
    a = net.architecture()
    assert (a["activation"], a["norm"], a["final_activation"]) == (1, 1, 4)
    for s, t, c in zip(a["scale"], a["shift"], net.channels[1:]):
        assert s.shape == (c,) and t.shape == (c,)
        np.testing.assert_allclose(s, 1 / np.sqrt(1 + 1e-5), rtol=1e-7)
        np.testing.assert_array_equal(t, 0)
    # statistics are parameters of the net, not constants of the kernels
    rng = np.random.default_rng(3)
    for p in net.batch_norm:
        for k in ("weight", "bias", "running_mean"):
            p[k] = rng.standard_normal(p[k].shape).astype(np.float32)
        p["running_var"] = rng.uniform(0.5, 2, p["running_var"].shape).astype(np.float32)
    a = net.architecture()
    x = rng.standard_normal((7, net.channels[1])).astype(np.float32)
    bn = torch.nn.BatchNorm1d(net.channels[1]).eval()
    p = net.batch_norm[0]
    with torch.no_grad():
        for k in ("weight", "bias"):
            getattr(bn, k).copy_(torch.from_numpy(p[k]))
        bn.running_mean.copy_(torch.from_numpy(p["running_mean"]))
        bn.running_var.copy_(torch.from_numpy(p["running_var"]))
        ref = bn(torch.from_numpy(x)).numpy()
    np.testing.assert_allclose(x * a["scale"][0] + a["shift"][0], ref, rtol=1e-5, atol=1e-5)
    assert AWAREDetectorNet(norm_layer="none").architecture()["scale"] is None


def test_load_with_an_edited_card(tmp_path):
    import yaml
    from aware_amd.utils.models import load
    card = yaml.safe_load(open(os.path.join(ROOT, "aware_amd", "cards", "config.yaml")))
    card["detection_net_cfg"] = dict(card["detection_net_cfg"], activation="swish", norm_layer="batch",
                                     final_activation="sigmoid")
    card["loss"] = "push_sigmoid"
    path = tmp_path / "config.yaml"
    path.write_text(yaml.safe_dump(card))
    out = load(str(path))
    assert out is not None
    emb, det = out
    assert det.detection_net is emb.detection_net
    net = emb.detection_net
    assert (net.activation, net.norm_layer, net.final_activation) == ("swish", "batch", "sigmoid")
    assert emb.loss.name == "push_sigmoid"
    card["detection_net_cfg"]["norm_layer"] = "layer"                  # the reference's ValueError -> load() reports None
    path.write_text(yaml.safe_dump(card))
    assert load(str(path)) is None


def test_remaining_refusals():
    from aware_amd.detection import AWAREDetectorNet
    from aware_amd.embedding.losses import get_loss_fn
    with pytest.raises(NotImplementedError, match="kernel_size"):
        AWAREDetectorNet(kernel_size=3, padding=1)
    with pytest.raises(NotImplementedError, match="stride"):
        AWAREDetectorNet(stride=2)
    with pytest.raises(NotImplementedError, match="initial pool"):
        AWAREDetectorNet(initial_pool_size=4, initial_pool_stride=4)
    with pytest.raises(NotImplementedError):
        get_loss_fn("bce")
    from aware_amd.detection import AWAREDetector
    from aware_amd.training import DetectorTrainer
    det = AWAREDetector(AWAREDetectorNet(activation="gelu"))
    with pytest.raises(NotImplementedError, match="architecture"):
        DetectorTrainer(det)


def test_abi_exports_the_architecture_entry_points():
    from aware_amd._lib import build_library, load_library, SIGNATURES
    build_library()
    lib = load_library()
    assert lib.aware_version() >= 320
    header = open(os.path.join(ROOT, "include", "aware_hip.h")).read()
    for name in ("aware_detector_create_ex", "aware_detector_is_card"):
        assert name in SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
    for enum, value in (("AWARE_ACT_SWISH", 3), ("AWARE_NORM_BATCH", 1), ("AWARE_NORM_NONE", 2), ("AWARE_FINAL_TANH", 4),
                        ("AWARE_FINAL_SIGMOID", 5)):
        assert re.search(r"#define %s %d\b" % (enum, value), header)
    # validation before any device work: no plan, bad enums
    from aware_amd._lib import DetectorArch
    import ctypes as C
    h = C.c_void_p()
    assert lib.aware_detector_create_ex(C.byref(h), None, None, 128, 4, None, None, None, C.byref(DetectorArch(0, 0, 4))) == -1
    assert lib.aware_detector_is_card(None) == -1


def test_fixture_covers_every_variant():
    f = np.load(FIXTURE)
    keys = variant_keys()
    want = {f"{a}_{n}_tanh" for a in BLOCK for n in ("instance", "batch", "none")}
    want |= {f"leaky_relu_instance_{fa}" for fa in FINAL}
    assert set(keys) == want
    for k in ("gelu_instance_tanh", "relu_batch_sigmoid"):
        assert f[f"traj/{k}/losses"].shape == (400,)


@pytest.mark.parametrize("key", variant_keys())
def test_float64_restatement_matches_the_reference(key):
    """The restatement the GPU tests use, against the reference's own float32 CPU outputs and magnitude gradients."""
    from aware_amd.detection import AWAREDetectorNet
    act, norm, fin = split_key(key)
    f = np.load(FIXTURE)
    net = AWAREDetectorNet(activation=act, norm_layer=norm, final_activation=fin)
    vd = VariantDetector(net)
    mag = torch.from_numpy(fixture_magnitudes()).double().requires_grad_(True)
    pred = vd.forward(mag)
    push_extremes_sum(pred, torch.from_numpy(f["target"]).double()).backward()
    np.testing.assert_allclose(pred.detach().numpy(), f[f"net/{key}/pred"][..., 0], atol=2e-6)
    g, ref = mag.grad.numpy()[:, 32:257, ::int(f["grad_step"])], f[f"net/{key}/grad"]     # the fixture keeps every 8th frame
    for b in range(g.shape[0]):
        rel = np.linalg.norm(g[b] - ref[b]) / np.linalg.norm(ref[b])
        assert rel < 1e-4, (key, b, rel)
