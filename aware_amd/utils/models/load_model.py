"""load(): (embedder, detector) from the YAML model card.

Reference: src/AWARE/utils/models/load_model.py:6-76.  Behaviour kept: every key is optional with the
reference's default, the detector is built around the embedder's own detection_net (:56), and a
failure at any stage is logged and reported as `None` instead of raising (:15-17, :45-49, :69-73)."""
from pathlib import Path

from ..logger import logger
from ..utils import load_config

_CARD = Path(__file__).resolve().parents[2] / "cards" / "config.yaml"

# constructor argument -> (card key, default); tuples for the band edges like the reference
_SHARED = {"frame_length": ("frame_length", 1024), "hop_length": ("hop_length", 256),
           "window": ("window", "hann"), "win_length": ("win_length", 1024),
           # EXTENSION: the embed / detect loop at any STFT geometry; absent = the card geometry only
           "general_geometry": ("general_geometry", False)}
_EMBEDDER = {"pattern_mode": ("pattern_mode", "bits2bipolar"), "tolerance_db": ("tolerance_db", 6.0),
             "num_iterations": ("num_iterations", 400), "detection_net_cfg": ("detection_net_cfg", {}),
             "optimizer_cfg": ("optimizer_cfg", {"name": "nadam", "params": {"lr": 0.1}}),
             "scheduler_cfg": ("scheduler_cfg", {"name": "reduce_lr_on_plateau", "params": {"factor": 0.9, "patience": 500}}),
             "loss": ("loss", "push_extremes"), "verbose": ("verbose", True),
             # EXTENSION (embedding/loop_attacks.py): attacks inside the optimisation loop; absent = none
             "loop_attacks": ("loop_attacks", None), "loop_attack_seed": ("loop_attack_seed", 0),
             # EXTENSION: one of several chains drawn per clip and step; absent = none, and not beside loop_attacks
             "loop_attack_mixture": ("loop_attack_mixture", None),
             # EXTENSION: loop_attacks of the element-wise kinds beside general_geometry; absent = refused there
             "general_loop_attacks": ("general_loop_attacks", False),
             # EXTENSION (utils/watermark/fec.py): the channel code of service.embed_message / detect_message; absent = none
             "payload_code": ("payload_code", None),
             # EXTENSION: kernel_size / stride / padding of detection_net_cfg; absent = 1x1 convolutions only
             "temporal_convs": ("temporal_convs", False),
             # EXTENSION: initial_pool_size / initial_pool_stride of detection_net_cfg; absent = (2, 2) only
             "initial_pools": ("initial_pools", False)}
_DETECTOR = {"threshold": ("threshold", 0.0), "pattern_mode": ("pattern_mode", "bipolar"),
             # EXTENSION (detection/sync.py): offset search in detection; absent = off
             "sync_search": ("sync_search", 0),
             # EXTENSION (detection/sync.py): speed search in detection; absent = off
             "speed_search": ("speed_search", None),
             # EXTENSION (detection/sync.py): shift search in detection; absent = off
             "shift_search": ("shift_search", None),
             # EXTENSION (detection/sync.py): the defaults of AWAREDetector.scan; absent = window_seconds 1.0,
             # hop_samples 4096, min_confidence 0.06, max_segments 16
             "scan": ("scan", None),
             # EXTENSION (utils/watermark/fec.py): as the embedder's
             "payload_code": ("payload_code", None)}


def _pick(card: dict, table: dict) -> dict:
    return {arg: card.get(key, default) for arg, (key, default) in table.items()}


def _stage(what, fn):
    try:
        return fn()
    except Exception as exc:                      # the reference swallows everything here
        logger.error(f"Error {what}: {exc}")
        return None


def load(config_path=None):
    from ...detection import AWAREDetector
    from ...embedding import AWAREEmbedder

    card = _stage("loading configs", lambda: load_config(config_path or _CARD))
    if card is None:
        return None
    bands = tuple(card.get("embedding_bands", [500, 4000]))
    embedder = _stage("creating embedder", lambda: AWAREEmbedder(
        embedding_bands=bands, **_pick(card, _SHARED), **_pick(card, _EMBEDDER)))
    if embedder is None:
        return None
    detector = _stage("creating detector", lambda: AWAREDetector(
        model=embedder.detection_net, embedding_bands=bands, **_pick(card, _SHARED), **_pick(card, _DETECTOR)))
    if detector is None:
        return None
    return embedder, detector
