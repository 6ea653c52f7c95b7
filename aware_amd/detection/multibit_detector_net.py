"""AWAREDetectorNet: frozen, seed-initialised detector (mel -> InstanceNorm -> global standardise
-> pool -> (num_blocks + 1) x [conv1d, norm, activation] -> bitwise read-out head with its final activation).
The model card's convolutions are 1x1; with the key temporal_convs every block is Conv1d(kernel_size, stride, padding)
along the pooled frames (aware_detector_create_conv), and with the key initial_pools the pool is
AvgPool1d(initial_pool_size, initial_pool_stride) for sizes and strides 2..8 (aware_detector_create_pool).

The model card's blocks are InstanceNorm + LeakyReLU with a tanh read-out; the other choices of the
reference's detection_net_cfg (activation, norm_layer, final_activation; modules/conv1d.py:8-36,
multibit_detector_net.py:82-96) run the staged route of the C ABI (aware_detector_create_ex).

Reference: src/AWARE/detection/multibit_detector_net.py:17-140.  The weights are never trained
anywhere in the reference (multibit_embedder.py:76-77 freezes them; there is no checkpoint), so
this class owns host copies generated from the reference's seed and a device copy inside
libaware_hip.so; forward() runs on the GPU through the C ABI."""
from __future__ import annotations

import numpy as np
import torch

from ..interfaces import BaseDetectorNet
from ..runtime import check_tap_clips, conv_rows, pool_rows
from .mel import mel_filter_bank

DETECTOR_SEED = 328656719      # multibit_detector_net.py:78

# Conv1dBlock._get_activation (modules/conv1d.py:27-36): an unknown name silently becomes ReLU
BLOCK_ACTIVATIONS = {"relu": 0, "leaky_relu": 1, "gelu": 2, "swish": 3}
# Conv1dBlock._get_norm_layer (:17-25)
NORM_LAYERS = {"instance": 0, "batch": 1, "none": 2}
# AWAREDetectorNet._get_activation (multibit_detector_net.py:82-96): anything else raises ValueError
FINAL_ACTIVATIONS = {"relu": 0, "leaky_relu": 1, "gelu": 2, "swish": 3, "tanh": 4, "sigmoid": 5}
CARD_ARCH = ("leaky_relu", "instance", "tanh")
BATCH_NORM_EPS = 1e-5          # nn.BatchNorm1d default


def block_activation(name: str) -> str:
    """The activation a Conv1dBlock builds for `name` (case-insensitive; unknown -> relu, as the reference)."""
    n = name.lower()
    return n if n in BLOCK_ACTIVATIONS else "relu"


def norm_layer_name(name: str) -> str:
    n = name.lower()
    if n not in NORM_LAYERS:
        raise ValueError(f"Invalid norm layer: {name}")
    return n


def final_activation_name(name: str) -> str:
    n = name.lower()
    if n not in FINAL_ACTIVATIONS:
        raise ValueError(f"Invalid activation: {name}")
    return n


# the longest payload the read-out kernels serve (aware_detector_create: a last block of at most 1024 channels)
MAX_OUTPUT_LENGTH = 512
# the largest mel bank, hidden width and depth aware_detector_create takes
MAX_N_MELS = 512
MAX_FILTERS = 4096
MAX_NUM_BLOCKS = 32
# the temporal convolutions aware_detector_create_conv takes (key temporal_convs): 2 * padding <= kernel_size - 1, so that no
# block is longer than its input
MAX_KERNEL_SIZE = 7
MAX_STRIDE = 4
# the initial pools aware_detector_create_pool takes (key initial_pools), size and stride alike.  From 2 on a clip of T frames
# has at most T // 2 pooled rows, what every batch allocates; a size or stride of 1 can give more
MIN_POOL = 2
MAX_POOL = 8


class AWAREDetectorNet(BaseDetectorNet):
    def __init__(self, sample_rate: int = 16000, n_fft: int = 1024, n_mels: int = 128,
                 initial_pool_size: int = 2, initial_pool_stride: int = 2, num_blocks: int = 3,
                 n_filters=(512, 1024, 1024), kernel_size: int = 1, stride: int = 1, padding: int = 0,
                 norm_layer: str = "instance", activation: str = "leaky_relu", output_length: int = 20,
                 final_activation: str = "tanh", temporal_convs: bool = False, initial_pools: bool = False):
        """initial_pools (EXTENSION; `initial_pools: true` in the card): serve initial_pool_size 2..8 and
        initial_pool_stride 2..8 in any combination.  Off, anything but (2, 2) raises NotImplementedError; on with (2, 2) the
        net is the same net on the same kernels.
        temporal_convs (EXTENSION; `temporal_convs: true` in the card): serve kernel_size 1..7,
        stride 1..4 and padding with 2 * padding <= kernel_size - 1 in every block.  Off, anything but 1 / 1 / 0 raises
        NotImplementedError; on with 1 / 1 / 0 the net is the same net on the same kernels."""
        n_filters = list(n_filters)
        assert len(n_filters) == num_blocks, "Number of filters must match number of blocks"
        # the reference's own validation, in its order: the blocks' norm layers (ValueError), then the final activation
        self.norm_layer = norm_layer_name(norm_layer)
        self.activation = block_activation(activation)
        self.final_activation = final_activation_name(final_activation)
        self.temporal_convs = bool(temporal_convs)
        unsupported = []
        if (kernel_size, stride, padding) != (1, 1, 0) and not self.temporal_convs:
            unsupported.append("kernel_size/stride/padding other than 1/1/0 (served with the key temporal_convs: "
                               "temporal_convs=True, or `temporal_convs: true` in the card)")
        self.initial_pools = bool(initial_pools)
        if (initial_pool_size, initial_pool_stride) != (2, 2) and not self.initial_pools:
            unsupported.append("initial pool other than (2, 2) (served with the key initial_pools: initial_pools=True, or "
                               "`initial_pools: true` in the card)")
        if unsupported:
            raise NotImplementedError("the HIP detector implements 1x1 convolutions after a (2, 2) pool only: " + "; ".join(unsupported))
        if self.temporal_convs:
            kernel_size, stride, padding = int(kernel_size), int(stride), int(padding)
            if kernel_size < 1 or stride < 1 or padding < 0:
                raise ValueError(f"kernel_size / stride / padding = {kernel_size} / {stride} / {padding}: kernel_size and "
                                 "stride must be positive and padding non-negative")
            if kernel_size > MAX_KERNEL_SIZE:
                raise NotImplementedError(f"kernel_size = {kernel_size}: temporal_convs serves kernel_size 1..{MAX_KERNEL_SIZE}")
            if stride > MAX_STRIDE:
                raise NotImplementedError(f"stride = {stride}: temporal_convs serves stride 1..{MAX_STRIDE}")
            if 2 * padding > kernel_size - 1:
                raise NotImplementedError(f"padding = {padding} with kernel_size = {kernel_size}: temporal_convs serves "
                                          "2 * padding <= kernel_size - 1 (no block longer than its input)")
        self.kernel_size, self.stride, self.padding = kernel_size, stride, padding
        if self.initial_pools:
            initial_pool_size, initial_pool_stride = int(initial_pool_size), int(initial_pool_stride)
            if initial_pool_size < 1 or initial_pool_stride < 1:
                raise ValueError(f"initial_pool_size / initial_pool_stride = {initial_pool_size} / {initial_pool_stride}: both "
                                 "must be positive")
            if not MIN_POOL <= initial_pool_size <= MAX_POOL:
                raise NotImplementedError(f"initial_pool_size = {initial_pool_size}: initial_pools serves initial_pool_size "
                                          f"{MIN_POOL}..{MAX_POOL}")
            if not MIN_POOL <= initial_pool_stride <= MAX_POOL:
                raise NotImplementedError(f"initial_pool_stride = {initial_pool_stride}: initial_pools serves "
                                          f"initial_pool_stride {MIN_POOL}..{MAX_POOL}")
        if n_mels < 1 or num_blocks < 0 or any(f < 1 for f in n_filters) or output_length < 1:
            raise ValueError(f"detector sizes must be positive: n_mels = {n_mels}, num_blocks = {num_blocks}, "
                             f"n_filters = {n_filters}, output_length = {output_length}")
        if n_mels > MAX_N_MELS:
            raise NotImplementedError(f"n_mels = {n_mels}: the HIP detector serves mel banks of at most {MAX_N_MELS} bands")
        if num_blocks > MAX_NUM_BLOCKS:
            raise NotImplementedError(f"num_blocks = {num_blocks}: the HIP detector serves at most {MAX_NUM_BLOCKS} blocks")
        if any(f > MAX_FILTERS for f in n_filters):
            raise NotImplementedError(f"n_filters = {n_filters}: the HIP detector serves blocks of at most {MAX_FILTERS} "
                                      "channels")
        if output_length > MAX_OUTPUT_LENGTH:
            raise NotImplementedError(f"output_length = {output_length}: the HIP detector reads out payloads of at most "
                                      f"{MAX_OUTPUT_LENGTH} bits (a last block of at most {2 * MAX_OUTPUT_LENGTH} channels)")
        self.sample_rate, self.n_fft, self.n_mels = sample_rate, n_fft, n_mels
        self.num_blocks, self.initial_pool_size, self.output_length = num_blocks, initial_pool_size, output_length
        self.initial_pool_stride = initial_pool_stride
        self.channels = [n_mels] + n_filters + [2 * output_length]
        self.mel_basis = mel_filter_bank(sample_rate, n_fft, n_mels)
        # torch.manual_seed(seed); self.apply(_init_weights): xavier-uniform on each Conv1d weight
        # in registration order, zero bias (:77-80, :98-107).  A private generator with the same
        # seed draws the same mt19937 stream without reseeding the caller's global RNG.
        gen = torch.Generator().manual_seed(DETECTOR_SEED)
        self.weights, self.biases = [], []
        # weights[i]: [cout, cin] for 1x1 convolutions, [cout, cin, kernel_size] for a net of temporal convolutions
        for cin, cout in zip(self.channels[:-1], self.channels[1:]):
            w = torch.empty(cout, cin, kernel_size)
            torch.nn.init.xavier_uniform_(w, generator=gen)
            self.weights.append((w if self.has_taps else w[:, :, 0]).contiguous().numpy())
            self.biases.append(np.zeros(cout, dtype=np.float32))
        # BatchNorm1d parameters and running statistics of every block (eval mode: both reference entry points call .eval());
        # a fresh net's values.  BatchNorm has no Conv / Linear weight, so the xavier draws above do not depend on the norm
        self.batch_norm = None
        if self.norm_layer == "batch":
            self.batch_norm = [{"weight": np.ones(c, np.float32), "bias": np.zeros(c, np.float32),
                                "running_mean": np.zeros(c, np.float32), "running_var": np.ones(c, np.float32),
                                "eps": BATCH_NORM_EPS} for c in self.channels[1:]]
        self._dev = None
        # the band the plug-in seam (forward) hands to the network: set by the embedder / detector that owns the net
        self.embedding_bands = None

    @property
    def has_taps(self) -> bool:
        """Whether the blocks are temporal convolutions (anything but kernel_size / stride / padding 1 / 1 / 0)."""
        return (self.kernel_size, self.stride, self.padding) != (1, 1, 0)

    @property
    def pool(self) -> tuple:
        """(initial_pool_size, initial_pool_stride)."""
        return (self.initial_pool_size, self.initial_pool_stride)

    @property
    def has_pool(self) -> bool:
        """Whether the initial pool is anything but the model card's (2, 2)."""
        return self.pool != (2, 2)

    @property
    def is_card_arch(self) -> bool:
        """Whether the blocks and the read-out are the model card's (the fused kernels); else the staged route, which a net
        of temporal convolutions or with another initial pool always takes."""
        return ((self.activation, self.norm_layer, self.final_activation) == CARD_ARCH and not self.has_taps
                and not self.has_pool)

    def pooled_rows(self, frames: int) -> int:
        """L_0: the rows a clip of `frames` STFT frames enters block 0 with (runtime.pool_rows)."""
        return pool_rows(int(frames), *self.pool)

    def block_rows(self, pooled_rows: int) -> list:
        """[L_0 .. L_{num_blocks + 1}]: the rows of a clip of L_0 pooled rows behind every block."""
        return [conv_rows(int(pooled_rows), i, self.kernel_size, self.stride, self.padding) for i in range(len(self.channels))]

    def check_clip_frames(self, who: str, frames):
        """ValueError naming the first clip (of `frames` STFT frames each) that the pool or some block leaves without a row,
        where torch's avg_pool1d / conv1d raise too; a net of 1x1 convolutions after the (2, 2) pool takes every clip."""
        check_tap_clips(who, frames, len(self.channels) - 1, (self.kernel_size, self.stride, self.padding), self.pool)

    def architecture(self):
        """The aware_detector_arch of this network: enum values, and for BatchNorm the folded eval-mode map
        scale = weight / sqrt(running_var + eps), shift = bias - running_mean * scale per block (computed in float64)."""
        arch = {"activation": BLOCK_ACTIVATIONS[self.activation], "norm": NORM_LAYERS[self.norm_layer],
                "final_activation": FINAL_ACTIVATIONS[self.final_activation], "scale": None, "shift": None}
        if self.batch_norm is not None:
            arch["scale"], arch["shift"] = [], []
            for bn in self.batch_norm:
                sc = np.asarray(bn["weight"], np.float64) / np.sqrt(np.asarray(bn["running_var"], np.float64) + bn["eps"])
                arch["scale"].append(sc.astype(np.float32))
                arch["shift"].append((np.asarray(bn["bias"], np.float64) -
                                      np.asarray(bn["running_mean"], np.float64) * sc).astype(np.float32))
        return arch

    def eval(self):
        return self

    def to(self, device):
        return self

    def parameters(self):
        for w, b in zip(self.weights, self.biases):
            yield w
            yield b
        for bn in self.batch_norm or ():
            yield bn["weight"]
            yield bn["bias"]

    def band_plan(self):
        """Card plan of the net's embedding band (`embedding_bands`, Hz at `sample_rate`; None: the default plan)."""
        from ..utils.audio import band_bins, default_plan, get_plan
        if self.embedding_bands is None:
            return default_plan()
        return get_plan(bins=band_bins(self.sample_rate, self.n_fft, self.embedding_bands))

    def device_weights(self, plan):
        """Device copy (aware_detector) bound to a plan; created on first use."""
        from ..runtime import DetectorWeights
        if self._dev is None or self._dev.plan is not plan:
            conv = (self.kernel_size, self.stride, self.padding) if self.has_taps else None
            self._dev = DetectorWeights(plan, self.mel_basis, self.weights, self.biases, arch=self.architecture(), conv=conv,
                                        pool=self.pool if self.has_pool else None)
        return self._dev

    def forward(self, stft_magnitude: torch.Tensor) -> torch.Tensor:
        """[B, n_fft/2+1, T] magnitudes -> [B, output_length, 1]  (net :109-140).

        Only the embedding band reaches the network (callers zero the rest,
        multibit_embedder.py:104, multibit_detector.py:34-37): `embedding_bands` (Hz, set by the
        AWAREEmbedder / AWAREDetector that owns the net), or 500-4000 Hz when it is None."""
        return _DetectorNetFn.apply(stft_magnitude.to("cuda", torch.float32), self)

    def get_model_info(self):
        total = int(sum(int(np.prod(p.shape)) for p in self.parameters()))
        return {"sample_rate": self.sample_rate, "n_fft": self.n_fft, "n_mels": self.n_mels,
                "num_blocks": self.num_blocks, "output_length": self.output_length,
                "activation": self.activation, "norm_layer": self.norm_layer,
                "final_activation": self.final_activation, "kernel_size": self.kernel_size, "stride": self.stride,
                "padding": self.padding, "initial_pool_size": self.initial_pool_size,
                "initial_pool_stride": self.initial_pool_stride, "total_parameters": total, "trainable_parameters": 0}


def _frames_batch(B, T):
    """Batch geometry with exactly T frames per clip (n = 256*(T-1) samples); cached."""
    from ..utils.audio import get_batch
    return get_batch([max(256 * (T - 1), 513)] * B)


def _band_rows(stft_magnitude, plan):
    """[B, F, T] -> frame-major band rows [B*T, plan.band_stride] (layout conversion at the seam)."""
    B, F, T = stft_magnitude.shape
    lo, hi = plan.band_bins
    mag = torch.zeros((B * T, plan.band_stride), dtype=torch.float32, device=stft_magnitude.device)
    mag[:, : hi - lo + 1] = stft_magnitude[:, lo:hi + 1, :].permute(0, 2, 1).reshape(B * T, -1)
    return mag


class _DetectorNetFn(torch.autograd.Function):
    """AWAREDetectorNet.forward under autograd (the reference back-propagates the loss through the frozen network to the
    magnitudes, multibit_embedder.py:107-111): forward = aware_detector_forward, backward = aware_detector_backward."""

    @staticmethod
    def forward(ctx, stft_magnitude, net):
        from .. import runtime as rt
        from ..utils.audio import default_plan
        plan = net.band_plan()
        B, F, T = stft_magnitude.shape
        batch = _frames_batch(B, T)
        mag = _band_rows(stft_magnitude, plan)
        ctx.save_for_backward(mag)
        ctx.geom = (plan, batch, net, (B, F, T))
        return rt.detector_forward(plan, net.device_weights(plan), batch, mag).unsqueeze(-1)

    @staticmethod
    def backward(ctx, g):
        from .. import runtime as rt
        (mag,) = ctx.saved_tensors
        plan, batch, net, (B, F, T) = ctx.geom
        _, gmag = rt.detector_backward(plan, net.device_weights(plan), batch, mag, g.reshape(B, -1))
        lo, hi = plan.band_bins
        out = torch.zeros((B, F, T), dtype=torch.float32, device=g.device)
        out[:, lo:hi + 1, :] = gmag[:, : hi - lo + 1].reshape(B, T, -1).permute(0, 2, 1)
        return out, None
