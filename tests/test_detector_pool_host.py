"""CPU tests of detectors with any initial pool (detection_net_cfg initial_pool_size / initial_pool_stride behind the key
initial_pools): the key on its three surfaces and the refusal that stays without it, load() of an edited
card, the range refusals, the row rule against torch's avg_pool1d and the library's own, the short-clip ValueError,
seed-identical weights, the search refusals, the C ABI's new symbols, and the float64 restatement the GPU tests hold the
kernels to (checked here against the reference's own outputs in tests/golden/detector_pool.npz, written by
tools/make_golden_pool.py)."""
import contextlib
import os
import re
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT
from test_detector_taps_host import KINK, TapDetector
from test_detector_variants_host import fixture_magnitudes, push_extremes_sum

FIXTURE = os.path.join(GOLDEN, "detector_pool.npz")


def pool(size, stride):
    return dict(initial_pool_size=size, initial_pool_stride=stride)


# detection_net_cfg edits of tools/make_golden_pool.py
CONFIGS = {
    "p44": pool(4, 4),
    "p32": pool(3, 2),
    "p23": pool(2, 3),
    "p82": pool(8, 2),
    "p88": pool(8, 8),
    "p33_small": dict(pool(3, 3), n_mels=80, num_blocks=2, n_filters=[72, 64], activation="gelu", norm_layer="batch",
                      final_activation="sigmoid"),
    "p44_k3": dict(pool(4, 4), kernel_size=3, stride=1, padding=1),
}
# the reference's own 400-step embeds in the fixture: name -> (clip samples, detection_net_cfg edit)
TRAJ = {"p44": (16000, pool(4, 4)), "p32": (48000, pool(3, 2))}
SERVED = [(size, stride) for size in range(2, 9) for stride in range(2, 9)]


def make_net(name, **kw):
    from aware_amd.detection import AWAREDetectorNet
    cfg = dict(CONFIGS[name], initial_pools=True, **kw)
    if (cfg.get("kernel_size", 1), cfg.get("stride", 1), cfg.get("padding", 0)) != (1, 1, 0):
        cfg["temporal_convs"] = True
    return AWAREDetectorNet(**cfg)


@contextlib.contextmanager
def restatement_pool(size, stride):
    """Inside, the AvgPool1d(2, 2) of the variant / tap restatement (its one call of F.avg_pool1d) is AvgPool1d(size, stride)."""
    real = torch.avg_pool1d

    def pooled(x, kernel_size, stride_):
        assert (kernel_size, stride_) == (2, 2), "the restatement's own pool call"
        return real(x, (size,), (stride,))

    with mock.patch.object(F, "avg_pool1d", pooled):
        yield


class PoolDetector(TapDetector):
    """TapDetector (VariantDetector for 1x1 blocks) with F.avg_pool1d(initial_pool_size, initial_pool_stride) as the pool
    between the mel stage and block 0 (multibit_detector_net.py:53, 131); everything else is that class's."""

    def pre_activations(self, mag):
        with restatement_pool(*self.net.pool):
            return super().pre_activations(mag)


# ---- the key -----------------------------------------------------------------------------------------------------------
def test_the_refusal_stays_without_the_key_and_names_it():
    from aware_amd.detection import AWAREDetectorNet
    from aware_amd.embedding import AWAREEmbedder
    for kw in (pool(4, 4), pool(3, 2), pool(2, 3), pool(1, 1)):
        for taps in (False, True):
            with pytest.raises(NotImplementedError, match="1x1 convolutions after a \\(2, 2\\) pool only") as e:
                AWAREDetectorNet(temporal_convs=taps, **kw)
            assert "initial pool other than (2, 2)" in str(e.value) and "initial_pools" in str(e.value)
    with pytest.raises(NotImplementedError, match="initial_pools"):
        AWAREEmbedder(detection_net_cfg=pool(4, 4), verbose=False)
    # both refusals in one message where both keys are missing
    with pytest.raises(NotImplementedError, match="temporal_convs.*initial_pools"):
        AWAREDetectorNet(kernel_size=3, **pool(4, 4))


def test_the_key_on_the_net_and_the_embedder():
    from aware_amd.detection import AWAREDetectorNet
    from aware_amd.embedding import AWAREEmbedder
    net = AWAREDetectorNet(initial_pools=True, **pool(4, 4))
    assert net.initial_pools and net.pool == (4, 4) and net.has_pool and not net.is_card_arch and not net.has_taps
    info = net.get_model_info()
    assert (info["initial_pool_size"], info["initial_pool_stride"]) == (4, 4) and info["total_parameters"] == 1681960
    emb = AWAREEmbedder(detection_net_cfg=pool(3, 2), initial_pools=True, verbose=False, loss="push_extremes")
    assert emb.initial_pools and emb.detection_net.pool == (3, 2) and emb.detection_net.initial_pools
    both = AWAREEmbedder(detection_net_cfg=dict(pool(4, 4), kernel_size=3, padding=1), initial_pools=True, temporal_convs=True,
                         verbose=False, loss="push_extremes")
    assert both.detection_net.pool == (4, 4) and both.detection_net.has_taps
    # the key with (2, 2): the card's net
    a, b = AWAREDetectorNet(), AWAREDetectorNet(initial_pools=True)
    assert b.pool == (2, 2) and not b.has_pool and b.is_card_arch
    for wa, wb in zip(a.weights, b.weights):
        np.testing.assert_array_equal(wa, wb)


def test_load_of_an_edited_card(tmp_path):
    import yaml
    from aware_amd.utils.models import load, load_model
    with open(load_model._CARD) as f:
        card = yaml.safe_load(f)
    assert "initial_pools" not in card
    card["detection_net_cfg"] = dict(card["detection_net_cfg"], **pool(4, 4))
    p = tmp_path / "no_key.yaml"
    p.write_text(yaml.safe_dump(card))
    assert load(str(p)) is None                                            # refused (load logs and returns None, as the reference)
    card["initial_pools"] = True
    p = tmp_path / "key.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, det = load(str(p))
    net = emb.detection_net
    assert emb.initial_pools and det.detection_net is net and net.pool == (4, 4) and net.has_pool
    assert [w.shape for w in net.weights] == [(512, 128), (1024, 512), (1024, 1024), (40, 1024)]
    # the key on the unedited card: the card's net
    with open(load_model._CARD) as f:
        card = yaml.safe_load(f)
    card["initial_pools"] = True
    p = tmp_path / "card_key.yaml"
    p.write_text(yaml.safe_dump(card))
    emb, _ = load(str(p))
    assert not emb.detection_net.has_pool and emb.detection_net.is_card_arch


def test_limits_and_their_messages():
    from aware_amd.detection import AWAREDetectorNet
    with pytest.raises(NotImplementedError, match="initial_pool_size = 9.*initial_pools serves initial_pool_size 2..8"):
        AWAREDetectorNet(initial_pools=True, **pool(9, 2))
    with pytest.raises(NotImplementedError, match="initial_pool_stride = 9.*initial_pools serves initial_pool_stride 2..8"):
        AWAREDetectorNet(initial_pools=True, **pool(2, 9))
    # size 1 and stride 1 stay refused: their rows can exceed floor(T / 2)
    with pytest.raises(NotImplementedError, match="initial_pool_size = 1.*2..8"):
        AWAREDetectorNet(initial_pools=True, **pool(1, 2))
    with pytest.raises(NotImplementedError, match="initial_pool_stride = 1.*2..8"):
        AWAREDetectorNet(initial_pools=True, **pool(2, 1))
    for bad in (pool(0, 2), pool(2, 0), pool(-1, 2), pool(2, -3)):
        with pytest.raises(ValueError, match="initial_pool_size / initial_pool_stride"):
            AWAREDetectorNet(initial_pools=True, **bad)
    for size, stride in SERVED:
        net = AWAREDetectorNet(initial_pools=True, num_blocks=0, n_filters=[], n_mels=8, **pool(size, stride))
        assert net.pool == (size, stride)


def test_pool_rows_matches_torch_and_the_library():
    """The Python mirror of pool_rows (and the library's own, where it is built) against the output length of
    torch.nn.functional.avg_pool1d for every served size and stride at T = 1..70; (2, 2) is T // 2 from T = 0; and no served
    pool gives more than T // 2 rows -- what the batch tables allocate."""
    from aware_amd import _lib
    from aware_amd.runtime import pool_rows
    lib = _lib.load_library() if os.path.exists(_lib.LIB_PATH) else None
    for size, stride in SERVED:
        for T in range(1, 71):
            try:
                want = F.avg_pool1d(torch.zeros(1, 1, T), size, stride).shape[-1]
            except RuntimeError:
                assert T < size
                want = 0                            # torch raises: no output row
            assert pool_rows(T, size, stride) == want, (size, stride, T)
            assert want <= T // 2
            if lib is not None:
                assert lib.aware_pool_rows(T, size, stride) == want
        assert pool_rows(0, size, stride) == 0
    for T in range(0, 71):
        assert pool_rows(T, 2, 2) == T // 2
        if lib is not None:
            assert lib.aware_pool_rows(T, 2, 2) == T // 2
    # why a size or stride of 1 is not served: more rows than the tables hold
    assert pool_rows(9, 1, 1) == 9 and pool_rows(9, 2, 1) == 8 and pool_rows(9, 1, 2) == 5 > 9 // 2
    if lib is not None:
        assert lib.aware_pool_rows(-1, 2, 2) == -1 and lib.aware_pool_rows(5, 0, 2) == -1 and lib.aware_pool_rows(5, 2, 0) == -1


def test_short_clip_value_error():
    """A clip that the pool, or a block behind it, leaves without a row: ValueError naming the clip, the stage and the rows,
    where clips are checked (no GPU needed)."""
    from aware_amd.detection import AWAREDetector, AWAREDetectorNet
    from aware_amd.embedding import AWAREEmbedder
    net = AWAREDetectorNet(initial_pools=True, **pool(8, 8))
    assert net.pooled_rows(63) == 7 and net.pooled_rows(8) == 1 and net.pooled_rows(7) == 0
    net.check_clip_frames("x", [63, 8])
    with pytest.raises(ValueError, match=r"x: clip 1 has 7 frames, and the initial pool .*size 8, stride 8.* leaves 0 rows"):
        net.check_clip_frames("x", [63, 7])
    emb = AWAREEmbedder(detection_net_cfg=pool(8, 8), initial_pools=True, verbose=False, loss="push_extremes")
    emb.check_clips([16000, 1792])                                         # 1 + 1792 // 256 = 8 frames: one row
    with pytest.raises(ValueError, match="AWAREEmbedder: clip 1 has 7 frames"):
        emb.check_clips([16000, 1791])
    det = AWAREDetector(emb.detection_net)
    with pytest.raises(ValueError, match="AWAREDetector: clip 0 has 7 frames"):
        det._check_tap_clips([1791])
    # a later block: pool (4, 4) leaves 4 rows of 19 frames, and the third block of kernel_size 3 none of its 0
    both = AWAREDetectorNet(initial_pools=True, temporal_convs=True, kernel_size=3, **pool(4, 4))
    assert both.block_rows(both.pooled_rows(19)) == [4, 2, 0, 0, 0]
    with pytest.raises(ValueError, match=r"clip 0 has 4 pooled rows \(19 frames\), and block 1 .*leaves 0 rows of its 2"):
        both.check_clip_frames("x", [19])
    AWAREDetector(AWAREDetectorNet(initial_pools=True))._check_tap_clips([600])     # (2, 2) takes every clip


@pytest.mark.parametrize("name", list(CONFIGS))
def test_seeded_weights_match_the_reference(name):
    """The pool has no weights: the draws are those of the same net after the (2, 2) pool, and their first values are the
    reference's conv_blocks[i].conv.weight."""
    fx = np.load(FIXTURE)
    net = make_net(name)
    assert tuple(fx[f"pool/{name}"]) == net.pool and net.has_pool and not net.is_card_arch
    first = fx[f"net/{name}/w_first"]
    assert first.shape[0] == len(net.weights) == net.num_blocks + 1
    same = make_net(name, initial_pool_size=2, initial_pool_stride=2)
    for i, w in enumerate(net.weights):
        np.testing.assert_array_equal(w.reshape(-1)[:first.shape[1]], first[i])
        np.testing.assert_array_equal(w, same.weights[i])
        assert not net.biases[i].any()


def test_fixture_holds_what_the_tests_read():
    fx = np.load(FIXTURE)
    assert list(fx["configs"]) == list(CONFIGS) and sorted(fx["traj"]) == sorted(TRAJ)
    assert os.path.getsize(FIXTURE) < 256 * 1024
    for name, (n, kw) in TRAJ.items():
        assert int(fx[f"traj/{name}/n"]) == n and tuple(fx[f"pool/{name}"]) == tuple(kw.values())
        assert fx[f"traj/{name}/losses"].shape == (400,)
        # the trajectories were picked where the reference reads its own payload back
        assert int(fx[f"traj/{name}/ber"]) == 0
        np.testing.assert_array_equal(np.asarray(fx[f"traj/{name}/det_bits"]).reshape(-1), fx[f"traj/{name}/bits"])


def test_searches_refuse_another_pool():
    """sync_search, speed_search, shift_search and scan: NotImplementedError naming the feature and the pool, at construction
    and per call; with (2, 2) and the key on they are taken as today."""
    from aware_amd.detection import AWAREDetector, AWAREDetectorNet
    net = AWAREDetectorNet(initial_pools=True, **pool(4, 4))
    for what, kw in (("sync_search", dict(sync_search=8)), ("speed_search", dict(speed_search=2.0)),
                     ("shift_search", dict(shift_search=20.0)), ("scan", dict(scan={"window_seconds": 1.0}))):
        with pytest.raises(NotImplementedError, match=what + r" is not supported with the initial pool \(size 4, stride 4\)") as e:
            AWAREDetector(net, **kw)
        assert "1024 samples" in str(e.value)
    det = AWAREDetector(net)
    clips = [np.zeros(16000, np.float32)]
    for what, call in (("sync_search", lambda: det.detect_batch(clips, 16000, sync_search=8)),
                       ("speed_search", lambda: det.detect_batch(clips, 16000, speed_search=2.0)),
                       ("shift_search", lambda: det.detect_batch_shift(clips, 16000, shift_search=20.0)),
                       ("scan", lambda: det.scan(clips, 16000))):
        with pytest.raises(NotImplementedError, match=what + " is not supported with the initial pool"):
            call()
    card = AWAREDetectorNet(initial_pools=True)
    d = AWAREDetector(card, sync_search=8, speed_search=2.0, scan={"window_seconds": 1.0})
    assert d.sync_search == 8 and d.speed_search is not None
    assert AWAREDetector(card, shift_search=20.0).shift_search is not None


def test_training_stays_refused():
    from aware_amd.detection import AWAREDetector
    from aware_amd.training import DetectorTrainer
    with pytest.raises(NotImplementedError, match="architecture"):
        DetectorTrainer(AWAREDetector(make_net("p44")))


def test_abi_symbols_and_signatures():
    from aware_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "aware_hip.h")).read()
    src = open(os.path.join(ROOT, "aware_amd", "csrc", "capi.hip")).read()
    for name, nargs in (("aware_detector_create_pool", 14), ("aware_detector_pool", 3), ("aware_pool_rows", 3)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert re.search(r"\bint %s\(" % name, hdr) and re.search(r'extern "C" int %s\(' % name, src)
    assert "mel_pool_kernels.hip" in _lib.SOURCES
    assert 'extern "C" int aware_version(void) { return 350; }' in src     # no version step: detected by symbol
    assert [f[0] for f in _lib.DetectorArch._fields_] == ["activation", "norm", "final_activation", "norm_scale", "norm_shift"]
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load_library()
        assert lib.aware_version() == 350
        assert lib.aware_pool_rows(63, 4, 4) == 15 and lib.aware_pool_rows(63, 8, 2) == 28 and lib.aware_pool_rows(7, 8, 8) == 0


# ---- the float64 restatement against the reference ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_float64_restatement_matches_the_reference(name):
    """PoolDetector in float64 against the reference's float32 CPU run: pred to 5e-5, the band gradient of push_extremes per
    clip to 2e-4 relative L2 (2e-2 for a clip with a ReLU / LeakyReLU argument within 1e-5 of 0: the bounds of
    tests/test_detector_taps_host.py)."""
    fx = np.load(FIXTURE)
    net = make_net(name)
    vd = PoolDetector(net)
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


def test_restatement_with_the_2_2_pool_is_the_tap_detector():
    from aware_amd.detection import AWAREDetectorNet
    net = AWAREDetectorNet(initial_pools=True)
    x = torch.from_numpy(fixture_magnitudes()).double()
    torch.testing.assert_close(PoolDetector(net).forward(x), TapDetector(net).forward(x), rtol=0, atol=0)
    # and the shim really pools: the rows of block 0 are pool_rows of the frames
    p44 = PoolDetector(make_net("p44"))
    assert p44.pre_activations(x)[0].shape[-1] == 15
