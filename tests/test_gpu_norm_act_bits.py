"""The conv block's tail (csrc/detector_kernels.hip: norm_act_fwd_kernel / norm_act_bwd_kernel, InstanceNorm over time or an
element-wise norm, then the activation, and their backward) keeps its bits when its kernels are restated: every result of a
detector call that passes through them is the same bit pattern as with aware_amd/csrc/ of the commit "Streaming STFT kernels:
single LDS reads, conflict-free LDS layouts", whose card blocks ran a second statement of the same maths (in_lrelu_*_kernel).

tests/golden/norm_act_parent_bits.json holds the sha256 of every array below and of each case's inputs, recorded on the
MI355X from that commit by `python tests/test_gpu_norm_act_bits.py OUT.json`.

Batches (hop 256, T = 1 + n // 256, pooled = T // 2; the launcher picks the form from the batch's longest clip):
  r32   [513, 32768, 65280]    1, 64 (unpaired last frame) and 128 pooled frames: R = 32 at its limit
  r80   [513, 33024, 163584]   1, 65 and 320: R = 80 with every register slot in use
  mem   [513, 164096]          1 and 321: from memory, next to a one-pooled-frame clip (the mul_rounded case)

Nets, and what det_plan gives them (every batch is ragged, so clip_tile_groups is 0 and no Clip kind applies):
  card96   the card's architecture with hidden widths 96 and 40: under 128 channels every block is Conv::Plain on every pipe, so
           each block's tail is norm_act_{fwd,bwd}_kernel<Instance, LeakyReLU, R> on one full and one partial group of 64
           channels (the `ok` mask).  In r32 / r80 the last block's forward is Conv::SplitK with the tail read-out, which hands
           down dL/dZ; in mem it is Plain with head_kernel, and its norm runs too.
  card     the model card's own net, r32 only.  aware_detector_forward / _backward run the f16 two-term pipe: blocks of 128
           channels and more take Conv::RaggedH2 with the norm in the GEMM epilogue, and none of these kernels.  The training
           entry runs the f32 pipe, where a ragged batch has no fused kind: every block Conv::Plain (the last one SplitK).
  leaky_relu_instance_sigmoid, gelu_instance_tanh, relu_instance_relu, swish_batch_tanh, relu_none_sigmoid
           variants: the staged route, Conv::Plain in every block and head_kernel.  <Instance, ., R> with a stash for GELU and
           ReLU, without for LeakyReLU; <Affine, Swish, 0> and <None, ReLU, 0> from memory at every length.
  taps_k3  temporal convolutions 3 / 1 / 1 on the card's architecture, widths 96 and 40: the staged route with the row rule
           inside the kernel (TAPS on; padding 1 keeps every block as long as its input)
  taps_1x1 the same net through aware_detector_create_conv at 1 / 1 / 0: the detector has no taps, is the card's, and runs
           what card96 runs (TAPS off)

Arrays per case: `values` of aware_detector_forward, `gmag` (dL/d|S|) of aware_detector_backward for a +-1 cotangent, and,
where the training entry serves the net (the card's architecture, 1x1 convolutions), `loss`, `pred`, `dW<l>` and `db<l>` of
aware_detector_train_gradients with push_extremes.  Every digest must be equal: a differing one is a changed contraction or
sum order in a kernel.

A kernel trace of this module shows norm_act_fwd_kernel and norm_act_bwd_kernel at <0, 1, 32 | 80 | 0, false> (card96, card,
taps_1x1, leaky_relu_instance_sigmoid), <0, 1, ., true> (taps_k3), <0, 0 | 2, 32 | 80 | 0, false>, <1, 3, 0, false> and
<2, 0, 0, false>, next to tail_kernel, head_kernel and the plain and ragged GEMMs, and no other kernel of a block's tail.

Run on the MI355X box:  python -m pytest tests/test_gpu_norm_act_bits.py -m gpu -q -s"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import GOLDEN  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "norm_act_parent_bits.json")
BATCHES = {"r32": [513, 32768, 65280], "r80": [513, 33024, 163584], "mem": [513, 164096]}
POOLED = {"r32": [1, 64, 128], "r80": [1, 65, 320], "mem": [1, 321]}
SEED = {"r32": 11, "r80": 12, "mem": 13}
VARIANTS = ["leaky_relu_instance_sigmoid", "gelu_instance_tanh", "relu_instance_relu", "swish_batch_tanh", "relu_none_sigmoid"]
SMALL = dict(num_blocks=2, n_filters=[96, 40])
NETS = {
    "card96": dict(SMALL),
    "card": dict(),
    "taps_k3": dict(SMALL, temporal_convs=True, kernel_size=3, stride=1, padding=1),
    "taps_1x1": dict(SMALL, temporal_convs=True, kernel_size=1, stride=1, padding=0),
}
CASES = [(net, b) for net in ["card96"] + VARIANTS + ["taps_k3", "taps_1x1"] for b in BATCHES] + [("card", "r32")]


@pytest.fixture(scope="module")
def rt():
    from aware_amd import runtime
    from aware_amd._lib import require_gpu
    require_gpu()
    return runtime


def make_net(name):
    from aware_amd.detection import AWAREDetectorNet
    if name in NETS:
        return AWAREDetectorNet(**NETS[name])
    act, norm, fin = name.rsplit("_", 2)
    return AWAREDetectorNet(activation=act, norm_layer=norm, final_activation=fin)


def sha(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


_INPUTS = {}


def inputs(rt, bname, nbits):
    """Band magnitude rows [total_frames, SPEC_STRIDE] of the batch and a +-1 payload / cotangent [B, nbits], on the host."""
    if (bname, nbits) not in _INPUTS:
        batch = rt.Batch(BATCHES[bname])
        assert [t // 2 for t in batch.frames] == POOLED[bname]
        rng = np.random.default_rng(SEED[bname])
        rows = torch.zeros((batch.total_frames, rt.SPEC_STRIDE), dtype=torch.float32)
        z = rng.standard_normal((batch.total_frames, 225, 2))
        rows[:, :225] = torch.from_numpy((0.3 * np.hypot(z[..., 0], z[..., 1])).astype(np.float32))
        target = torch.from_numpy(np.where(rng.integers(0, 2, (batch.B, nbits)) > 0, 1.0, -1.0).astype(np.float32))
        _INPUTS[bname, nbits] = (batch, rows, target)
    return _INPUTS[bname, nbits]


def run(rt, net_name, bname):
    """{array name: host tensor} of one case."""
    from aware_amd.utils.audio import default_plan
    plan = default_plan()
    net = make_net(net_name)
    dev = net.device_weights(plan)
    assert dev.is_card == (net_name in ("card96", "card", "taps_1x1"))
    batch, rows, target = inputs(rt, bname, net.output_length)
    rows, target = rows.cuda(), target.cuda()
    r = {"values": rt.detector_forward(plan, dev, batch, rows)}
    r["gmag"] = rt.detector_backward(plan, dev, batch, rows, target)[1]
    if dev.is_card and rt.training_refusal(dev.channels) is None:
        r["pred"], r["loss"], gw, gb = rt.detector_train_gradients(plan, dev, batch, rows, target, "push_extremes")
        for l, (w, b) in enumerate(zip(gw, gb)):
            r[f"dW{l}"], r[f"db{l}"] = w, b
    torch.cuda.synchronize()
    r = {k: v.cpu() for k, v in r.items()}
    for k, v in r.items():
        assert bool(torch.isfinite(v).all()), (net_name, bname, k)
    assert float(r["gmag"].abs().max()) > 0.0
    return r


def digests(rt):
    out = {"inputs": {}, "sha256": {}}
    for net_name, bname in CASES:
        _, rows, target = inputs(rt, bname, make_net(net_name).output_length)
        out["inputs"][f"{net_name}/{bname}"] = sha(torch.cat([rows.ravel(), target.ravel()]))
        out["sha256"][f"{net_name}/{bname}"] = {k: sha(v) for k, v in run(rt, net_name, bname).items()}
    return out


@pytest.fixture(scope="module")
def want():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_case(want):
    assert sorted(want["sha256"]) == sorted(f"{n}/{b}" for n, b in CASES)
    assert sorted(want["inputs"]) == sorted(want["sha256"])
    for key, arrays in want["sha256"].items():
        trains = key.split("/")[0] in ("card96", "card", "taps_1x1")
        assert ("loss" in arrays) == trains and ("dW0" in arrays) == trains, key


@pytest.mark.parametrize("net_name,bname", CASES)
def test_block_tail_keeps_the_parent_bits(rt, want, net_name, bname):
    key = f"{net_name}/{bname}"
    _, rows, target = inputs(rt, bname, make_net(net_name).output_length)
    assert sha(torch.cat([rows.ravel(), target.ravel()])) == want["inputs"][key], "the inputs differ, not the kernels"
    r = run(rt, net_name, bname)
    assert sorted(r) == sorted(want["sha256"][key])
    bad = [k for k in sorted(r) if sha(r[k]) != want["sha256"][key][k]]
    assert not bad, (key, bad)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from aware_amd import runtime
    with open(sys.argv[1], "w") as f:
        json.dump(digests(runtime), f, indent=0, sort_keys=True)
    print("wrote", sys.argv[1])
