"""CPU tests of detectors with temporal convolutions (detection_net_cfg kernel_size / stride / padding behind the key
temporal_convs): the key and the refusal that stays without it, seed-identical weights, the row rule against torch's conv1d,
the limits, the short-clip ValueError, load() of an edited card, the C ABI's new symbols, and the float64 restatement the GPU
tests hold the kernels to (checked here against the reference's own outputs in tests/golden/detector_taps.npz, written by
tools/make_golden_taps.py), with the torch statement of unfold and fold and their adjointness."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT
from test_detector_variants_host import VariantDetector, fixture_magnitudes, push_extremes_sum

FIXTURE = os.path.join(GOLDEN, "detector_taps.npz")
KINK = 1e-5

# detection_net_cfg edits of tools/make_golden_taps.py
CONFIGS = {
    "k3": dict(kernel_size=3),
    "k3_same": dict(kernel_size=3, padding=1),
    "k2": dict(kernel_size=2),
    "k5_p1": dict(kernel_size=5, padding=1, num_blocks=2, n_filters=[256, 256]),
    "k3_s2": dict(kernel_size=3, stride=2, padding=1, num_blocks=1, n_filters=[512]),
    "k4_s3": dict(kernel_size=4, stride=3, padding=1, num_blocks=1, n_filters=[250]),
    "k3_odd": dict(kernel_size=3, n_mels=13, num_blocks=2, n_filters=[30, 61], output_length=7),
    "k3_gelu_batch_sigmoid": dict(kernel_size=3, padding=1, n_mels=64, num_blocks=2, n_filters=[100, 202], activation="gelu",
                                  norm_layer="batch", final_activation="sigmoid"),
    "k7_p3": dict(kernel_size=7, padding=3, num_blocks=1, n_filters=[128]),
}
TRAJ = {
    "k3": (16000, dict(kernel_size=3)),
    "k3_s2": (48000, dict(kernel_size=3, stride=2, padding=1, num_blocks=2, n_filters=[256, 256])),
}
# every (kernel_size, stride, padding) of CONFIGS
KSP = sorted({(c["kernel_size"], c.get("stride", 1), c.get("padding", 0)) for c in CONFIGS.values()})


def served():
    """Every (k, s, p) the key serves: k 1..7, s 1..4, 2 p <= k - 1."""
    return [(k, s, p) for k in range(1, 8) for s in range(1, 5) for p in range(0, (k - 1) // 2 + 1)]


def make_net(name, **kw):
    from aware_amd.detection import AWAREDetectorNet
    return AWAREDetectorNet(**dict(CONFIGS[name], temporal_convs=True, **kw))


class TapDetector(VariantDetector):
    """VariantDetector with every block a Conv1d(kernel_size, stride, padding) along the pooled frames (modules/conv1d.py):
    weights [cout, cin, k]; the norms and the read-out mean run over the block's own rows."""

    def pre_activations(self, mag):
        net = self.net
        x = self.instance_norm(torch.matmul(self.mel, mag))
        x = (x - x.mean(dim=(1, 2), keepdim=True)) / (x.std(dim=(1, 2), keepdim=True) + 1e-8)
        x = F.avg_pool1d(x, 2, 2)
        us = []
        for l, (w, b) in enumerate(zip(self.ws, self.bs)):
            w3 = w if w.dim() == 3 else w[:, :, None]
            z = F.conv1d(x, w3, b, stride=net.stride, padding=net.padding)
            if net.norm_layer == "instance":
                u = self.instance_norm(z)
            elif net.norm_layer == "batch":
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


def unfold_rows(x, L_out, k, s, p):
    """The torch statement of the unfold on one clip: x [L_in, C] -> U [L_out, k C], U[t, j C + c] = x[t s - p + j, c] inside
    the clip, else 0."""
    L_in, C = x.shape
    u = torch.zeros((L_out, k * C), dtype=x.dtype)
    for t in range(L_out):
        for j in range(k):
            q = t * s - p + j
            if 0 <= q < L_in:
                u[t, j * C:(j + 1) * C] = x[q]
    return u


def fold_rows(du, L_in, k, s, p):
    """The torch statement of the fold: dU [L_out, k C] -> dX [L_in, C], the sum over j ascending of dU[t, j C + c] with
    t s - p + j = q."""
    L_out, C = du.shape[0], du.shape[1] // k
    dx = torch.zeros((L_in, C), dtype=du.dtype)
    for q in range(L_in):
        for j in range(k):
            e = q + p - j
            if e >= 0 and e % s == 0 and e // s < L_out:
                dx[q] = dx[q] + du[e // s, j * C:(j + 1) * C]
    return dx


# ---- the key -----------------------------------------------------------------------------------------------------------
def test_the_refusal_stays_without_the_key_and_names_it():
    from aware_amd.detection import AWAREDetectorNet
    for kw in (dict(kernel_size=3), dict(kernel_size=3, padding=1), dict(stride=2), dict(padding=1)):
        with pytest.raises(NotImplementedError, match="1x1 convolutions after a \\(2, 2\\) pool only") as e:
            AWAREDetectorNet(**kw)
        assert "temporal_convs" in str(e.value) and "kernel_size/stride/padding" in str(e.value)
    # the initial pool keeps its own refusal, with and without the key
    for key in (False, True):
        with pytest.raises(NotImplementedError, match="initial pool"):
            AWAREDetectorNet(initial_pool_size=4, initial_pool_stride=4, temporal_convs=key)


def test_the_key_with_1_1_0_is_the_same_net():
    from aware_amd.detection import AWAREDetectorNet
    a, b = AWAREDetectorNet(), AWAREDetectorNet(temporal_convs=True)
    assert not b.has_taps and b.is_card_arch and a.is_card_arch
    assert [w.shape for w in b.weights] == [w.shape for w in a.weights] == [(512, 128), (1024, 512), (1024, 1024), (40, 1024)]
    for wa, wb in zip(a.weights, b.weights):
        np.testing.assert_array_equal(wa, wb)
    assert a.get_model_info()["total_parameters"] == b.get_model_info()["total_parameters"] == 1681960


@pytest.mark.parametrize("name", list(CONFIGS))
def test_seeded_weights_match_the_reference(name):
    """weights[i] is [cout, cin, k] and its first values are the reference's conv_blocks[i].conv.weight (same seed, same
    draw order, fan-in cin k)."""
    fx = np.load(FIXTURE)
    net = make_net(name)
    k = net.kernel_size
    assert net.has_taps and not net.is_card_arch
    first = fx[f"net/{name}/w_first"]
    assert first.shape[0] == len(net.weights) == net.num_blocks + 1
    for i, w in enumerate(net.weights):
        assert w.shape == (net.channels[i + 1], net.channels[i], k) and w.dtype == np.float32
        np.testing.assert_array_equal(w.reshape(-1)[:first.shape[1]], first[i])
        assert not net.biases[i].any()
    info = net.get_model_info()
    # cout * cin * k + cout per block, and BatchNorm's weight and bias where the blocks have one
    want = sum(co * ci * k + co for ci, co in zip(net.channels[:-1], net.channels[1:]))
    want += 2 * sum(net.channels[1:]) if net.norm_layer == "batch" else 0
    assert info["total_parameters"] == want
    assert (info["kernel_size"], info["stride"], info["padding"]) == (net.kernel_size, net.stride, net.padding)


def test_conv_rows_matches_torch_conv1d():
    """The Python mirror of conv_rows (and the library's own, where it is built) against the output length of
    torch.nn.functional.conv1d for every served k, s, p at L = 1..70, through four blocks."""
    from aware_amd.detection.multibit_detector_net import conv_rows
    lib = None
    from aware_amd import _lib
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load_library()
    for k, s, p in served():
        w = torch.zeros(1, 1, k)
        # one block by torch, for every input length (a block never grows, so four blocks stay inside the table)
        one = {0: 0}
        for L in range(1, 71):
            try:
                one[L] = F.conv1d(torch.zeros(1, 1, L), w, stride=s, padding=p).shape[-1]
            except RuntimeError:
                assert L + 2 * p < k
                one[L] = 0                          # torch raises: no output row
        for L in range(1, 71):
            rows = [L]
            for blk in range(1, 5):
                rows.append(one[rows[-1]])
                assert conv_rows(L, blk, k, s, p) == rows[blk], (k, s, p, L, blk)
                assert rows[blk] <= rows[blk - 1]   # no block is longer than its input
                if lib is not None:
                    assert lib.aware_conv_rows(L, blk, k, s, p) == rows[blk]
            assert conv_rows(L, 0, k, s, p) == L


def test_limits_and_their_messages():
    from aware_amd.detection import AWAREDetectorNet
    with pytest.raises(NotImplementedError, match="kernel_size = 8.*temporal_convs serves kernel_size 1..7"):
        AWAREDetectorNet(kernel_size=8, temporal_convs=True)
    with pytest.raises(NotImplementedError, match="stride = 5.*temporal_convs serves stride 1..4"):
        AWAREDetectorNet(stride=5, temporal_convs=True)
    with pytest.raises(NotImplementedError, match="padding = 2 with kernel_size = 3.*2 \\* padding <= kernel_size - 1"):
        AWAREDetectorNet(kernel_size=3, padding=2, temporal_convs=True)
    with pytest.raises(NotImplementedError, match="padding = 1 with kernel_size = 2"):
        AWAREDetectorNet(kernel_size=2, padding=1, temporal_convs=True)
    for bad in (dict(kernel_size=0), dict(stride=0), dict(padding=-1)):
        with pytest.raises(ValueError, match="kernel_size / stride / padding"):
            AWAREDetectorNet(temporal_convs=True, **bad)
    for k, s, p in served():
        if k * 128 * 512 <= 2 ** 19:              # (keep the draw of the seeded weights small)
            AWAREDetectorNet(kernel_size=k, stride=s, padding=p, temporal_convs=True, num_blocks=0, n_filters=[], n_mels=8)


def test_short_clip_value_error():
    """A clip that some block leaves without a row: ValueError naming the clip, the block and the rows, where clips are
    checked (no GPU needed)."""
    from aware_amd.detection import AWAREDetector, AWAREDetectorNet
    from aware_amd.embedding import AWAREEmbedder
    net = AWAREDetectorNet(kernel_size=3, temporal_convs=True)            # four blocks: 2 rows less each, L0 >= 9 needed
    assert net.block_rows(31) == [31, 29, 27, 25, 23]
    assert net.block_rows(8) == [8, 6, 4, 2, 0]
    net.check_clip_frames("x", [63, 19])                                   # L0 = 9: one row left
    with pytest.raises(ValueError, match=r"clip 1 has 8 pooled rows \(17 frames\), and block 3 .*leaves 0 rows of its 2"):
        net.check_clip_frames("x", [63, 17])
    emb = AWAREEmbedder(detection_net_cfg=dict(kernel_size=3), temporal_convs=True, verbose=False, loss="push_extremes")
    emb.check_clips([16000, 4864])                                         # 1 + 4864 // 256 = 20 frames, L0 = 10
    with pytest.raises(ValueError, match="AWAREEmbedder: clip 1 has 8 pooled rows"):
        emb.check_clips([16000, 4100])
    det = AWAREDetector(emb.detection_net)
    with pytest.raises(ValueError, match="AWAREDetector: clip 0 has 8 pooled rows"):
        det._check_tap_clips([4100])
    AWAREDetector(AWAREDetectorNet())._check_tap_clips([600])              # 1x1 convolutions take every clip
    # the strided four-block net of the issue's last row still runs on a 1 s clip (31 -> 16 -> 8 -> 4 -> 2): not refused
    assert AWAREDetectorNet(kernel_size=3, stride=2, padding=1, temporal_convs=True).block_rows(31) == [31, 16, 8, 4, 2]


def test_load_of_an_edited_card(tmp_path):
    import yaml
    from aware_amd.utils.models import load, load_model
    with open(load_model._CARD) as f:
        card = yaml.safe_load(f)
    assert "temporal_convs" not in card
    card["detection_net_cfg"] = dict(card["detection_net_cfg"], kernel_size=3, stride=2, padding=1, num_blocks=2,
                                     n_filters=[256, 256])
    p = tmp_path / "no_key.yaml"
    p.write_text(yaml.safe_dump(card))
    assert load(str(p)) is None                                            # refused (load logs and returns None, as the reference)
    card["temporal_convs"] = True
    p = tmp_path / "key.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    net = emb.detection_net
    assert emb.temporal_convs and det.detection_net is net
    assert (net.kernel_size, net.stride, net.padding) == (3, 2, 1) and net.has_taps
    assert [w.shape for w in net.weights] == [(256, 128, 3), (256, 256, 3), (40, 256, 3)]
    # the key on the unedited card: the card's net
    with open(load_model._CARD) as f:
        card = yaml.safe_load(f)
    card["temporal_convs"] = True
    p = tmp_path / "card_key.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, _ = load(str(p))
    assert not emb.detection_net.has_taps and emb.detection_net.is_card_arch


def test_abi_symbols_and_signatures():
    from aware_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "aware_hip.h")).read()
    src = open(os.path.join(ROOT, "aware_amd", "csrc", "capi.hip")).read()
    for name, nargs in (("aware_detector_create_conv", 12), ("aware_detector_conv", 4), ("aware_conv_rows", 5),
                        ("aware_conv_unfold", 9), ("aware_conv_fold", 9)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert re.search(r"\bint %s\(" % name, hdr) and re.search(r'extern "C" int %s\(' % name, src)
    assert "conv_taps_kernels.hip" in _lib.SOURCES
    assert 'extern "C" int aware_version(void) { return 350; }' in src     # no version step: detected by symbol
    # aware_detector_arch is part of a pinned ABI: five fields, unchanged
    assert [f[0] for f in _lib.DetectorArch._fields_] == ["activation", "norm", "final_activation", "norm_scale", "norm_shift"]
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load_library()
        assert lib.aware_conv_rows(31, 4, 3, 1, 0) == 23 and lib.aware_conv_rows(93, 3, 3, 2, 1) == 12
        assert lib.aware_conv_rows(8, 4, 3, 1, 0) == 0 and lib.aware_conv_rows(-1, 1, 3, 1, 0) == -1


def test_training_stays_refused():
    from aware_amd.detection import AWAREDetector
    from aware_amd.training import DetectorTrainer
    with pytest.raises(NotImplementedError, match="architecture"):
        DetectorTrainer(AWAREDetector(make_net("k3")))


# ---- the float64 restatement against the reference ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_float64_restatement_matches_the_reference(name):
    """TapDetector in float64 against the reference's float32 CPU run: pred to 5e-5, the band gradient of push_extremes per
    clip to 2e-4 relative L2 (2e-2 for a clip with a ReLU / LeakyReLU argument within 1e-5 of 0: the bounds of
    tests/test_gpu_detector_sizes.py)."""
    fx = np.load(FIXTURE)
    net = make_net(name)
    vd = TapDetector(net)
    x = torch.from_numpy(fixture_magnitudes()).double()
    kink = vd.kink_distance(x)
    step = int(fx["grad_step"])
    for b in range(x.shape[0]):
        xb = x[b:b + 1].clone().requires_grad_(True)                       # one clip per call, as the reference's loops
        pred = vd.forward(xb)
        np.testing.assert_allclose(pred.detach().numpy()[0], fx[f"net/{name}/pred"][b, :, 0], atol=5e-5)
        push_extremes_sum(pred, torch.from_numpy(fx[f"net/{name}/target"][b:b + 1]).double()).backward()
        g, ref = xb.grad.numpy()[0, 32:257, ::step], fx[f"net/{name}/grad"][b]
        rel = np.linalg.norm(g - ref) / np.linalg.norm(ref)
        print(f"{name} clip {b}: pred err {np.max(np.abs(pred.detach().numpy()[0] - fx[f'net/{name}/pred'][b, :, 0])):.1e}, "
              f"gradient rel L2 {rel:.2e} (kink {kink[b]:.1e})")
        assert rel < (2e-4 if kink[b] > KINK else 2e-2)


def test_restatement_with_1x1_weights_is_the_variant_detector():
    from aware_amd.detection import AWAREDetectorNet
    net = AWAREDetectorNet(temporal_convs=True)
    x = torch.from_numpy(fixture_magnitudes()).double()
    torch.testing.assert_close(TapDetector(net).forward(x), VariantDetector(net).forward(x), rtol=0, atol=1e-12)


@pytest.mark.parametrize("k,s,p", KSP)
def test_unfold_is_conv1d_and_fold_is_its_adjoint(k, s, p):
    """float64: the unfolded rows times the weights laid out [cout, k cin] are F.conv1d, and <unfold x, u> = <x, fold u>."""
    from aware_amd.detection.multibit_detector_net import conv_rows
    g = torch.Generator().manual_seed(100 * k + 10 * s + p)
    C, Co = 8, 5
    for L_in in (1, 2, 3, 7, 31, 32, 33):
        L_out = conv_rows(L_in, 1, k, s, p)
        if L_out < 1:
            continue
        x = torch.randn(L_in, C, generator=g, dtype=torch.float64)
        w = torch.randn(Co, C, k, generator=g, dtype=torch.float64)
        U = unfold_rows(x, L_out, k, s, p)
        wg = w.permute(0, 2, 1).reshape(Co, k * C)                         # Wg[co][j C + ci] = W[co][ci][j]
        z = F.conv1d(x.T[None], w, stride=s, padding=p)[0].T
        assert z.shape == (L_out, Co)
        torch.testing.assert_close(U @ wg.T, z, rtol=1e-12, atol=1e-12)
        u = torch.randn(L_out, k * C, generator=g, dtype=torch.float64)
        lhs, rhs = (U * u).sum(), (x * fold_rows(u, L_in, k, s, p)).sum()
        assert abs(float(lhs - rhs)) <= 1e-12 * max(1.0, abs(float(lhs)))
