"""detect_watermark (reference: src/AWARE/service/detect.py:7-55): 16 kHz only, mono 1-D or
stereo [N,2] (per bit, the channel with the larger |value| wins, :23-37), then PatternDecoder.
EXTENSION: sync_search = n runs the detector's offset search (detection/sync.py); None keeps the detector's own setting.
EXTENSION: speed_search runs its speed search (same module), likewise."""
import numpy as np

from ..utils.logger import logger
from ..utils.watermark import PatternDecoder


def _searches(detector, sync_search, speed_search) -> bool:
    """Whether a search is asked for, here or by the detector."""
    return (sync_search is not None or speed_search is not None or bool(getattr(detector, "sync_search", 0))
            or bool(getattr(detector, "speed_search", None)))


def _detect(detector, clips, sample_rate, sync_search, speed_search=None):
    """detect_batch, through the searches that are asked for (here or by the detector); the plain call otherwise.  The
    speed search's keyword goes only to a detector that is asked for it."""
    if not _searches(detector, sync_search, speed_search):
        return detector.detect_batch(clips, sample_rate)
    if speed_search is None and not getattr(detector, "speed_search", None):
        vals, offsets, conf = detector.detect_batch(clips, sample_rate, sync_search=sync_search, return_sync=True)
        logger.debug(f"sync search: offsets {offsets.cpu().tolist()} samples, confidence {[round(float(c), 4) for c in conf.cpu()]}")
        return vals
    vals, offsets, m, conf = detector.detect_batch(clips, sample_rate, sync_search=sync_search, speed_search=speed_search,
                                                   return_speed=True)
    logger.debug(f"speed search: speed offsets {m.cpu().tolist()} / 65536, offsets {offsets.cpu().tolist()} samples, confidence "
                 f"{[round(float(c), 4) for c in conf.cpu()]}")
    return vals


def detect_watermark(audio: np.ndarray, sample_rate: int, detector, sync_search=None, speed_search=None):
    decode = PatternDecoder(encoder_mode=detector.pattern_mode, threshold=detector.threshold)
    if sample_rate != 16000:
        logger.error(f"Invalid sample rate. Expected 16000Hz, got {sample_rate}Hz.")
        raise ValueError("Invalid sample rate. Expected 16000Hz.")
    audio = np.asarray(audio)
    if audio.ndim == 2 and audio.shape[1] == 2:
        vals = _detect(detector, [audio[:, 0].astype(np.float32), audio[:, 1].astype(np.float32)], sample_rate, sync_search,
                       speed_search)
        l, r = vals[0].cpu().numpy(), vals[1].cpu().numpy()
        return decode(np.where(np.abs(l) > np.abs(r), l, r))
    if audio.ndim == 1:
        if not _searches(detector, sync_search, speed_search):
            return decode(detector.detect(audio, sample_rate))
        return decode(_detect(detector, [audio.astype(np.float32)], sample_rate, sync_search, speed_search)[0].detach().cpu().numpy())
    logger.error("Invalid audio shape. Expected 1D or 2D numpy array.")
    raise ValueError("Invalid audio shape. Expected 1D or 2D numpy array.")


def detect_watermark_batch(clips, sample_rate: int, detector, sync_search=None, speed_search=None):
    if sample_rate != 16000:
        raise ValueError("Invalid sample rate. Expected 16000Hz.")
    decode = PatternDecoder(encoder_mode=detector.pattern_mode, threshold=detector.threshold)
    vals = _detect(detector, [np.asarray(c, dtype=np.float32) for c in clips], sample_rate, sync_search, speed_search).cpu().numpy()
    return [decode(v) for v in vals]
