"""detect_watermark (reference: src/AWARE/service/detect.py:7-55): 16 kHz only, mono 1-D or
stereo [N,2] (per bit, the channel with the larger |value| wins, :23-37), then PatternDecoder.
EXTENSION: sync_search = n runs the detector's offset search (detection/sync.py); None keeps the detector's own setting.
EXTENSION: speed_search runs its speed search (same module), likewise.
EXTENSION: a detector with shift_search on (the card key) runs its shift search in every function here.
EXTENSION: scan_watermark reads a long recording in windows and returns its marked spans, one payload each (same module).
EXTENSION: detect_message reads the message of a coded payload (utils/watermark/fec.py), and with a
payload_code on the detector every span of a scan carries its decoded message."""
import numpy as np

from ..utils.logger import logger
from ..utils.watermark import PatternDecoder


def _searches(detector, sync_search, speed_search) -> bool:
    """Whether a search is asked for, here or by the detector."""
    return (sync_search is not None or speed_search is not None or bool(getattr(detector, "sync_search", 0))
            or bool(getattr(detector, "speed_search", None)) or bool(getattr(detector, "shift_search", None)))


def _detect(detector, clips, sample_rate, sync_search, speed_search=None):
    """detect_batch, through the searches that are asked for (here or by the detector); the plain call otherwise.  The
    speed search's keyword goes only to a detector that is asked for it."""
    if not _searches(detector, sync_search, speed_search):
        return detector.detect_batch(clips, sample_rate)
    if getattr(detector, "shift_search", None) and speed_search is None:
        vals, offsets, d, conf = detector.detect_batch_shift(clips, sample_rate, sync_search=sync_search, return_shift=True)
        logger.debug(f"shift search: shifts {d.cpu().tolist()} x {sample_rate} / 2^20 Hz, offsets {offsets.cpu().tolist()} samples, "
                     f"confidence {[round(float(c), 4) for c in conf.cpu()]}")
        return vals
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


def _scan(detector, files, sample_rate, options):
    if sample_rate != 16000:
        logger.error(f"Invalid sample rate. Expected 16000Hz, got {sample_rate}Hz.")
        raise ValueError("Invalid sample rate. Expected 16000Hz.")
    decode = PatternDecoder(encoder_mode=detector.pattern_mode, threshold=detector.threshold)
    found = detector.scan([np.asarray(f, dtype=np.float32) for f in files], sample_rate, **options)
    coded = ("message", "valid", "corrected")                   # what a detector with a payload_code adds to a span
    return [[dict({"start": s["start"], "end": s["end"], "peak": s["peak"], "confidence": s["confidence"],
                   "payload": decode(s["values"]), "values": s["values"]}, **{k: s[k] for k in coded if k in s})
             for s in spans] for spans in found]


def _scan_stereo(left, right, max_flip: int, centre: float = 0.0):
    """detect_watermark's rule for the spans of two channels.  A span's counterpart is the span of the other channel that it
    overlaps by the most samples (the earlier one on a tie).  Two spans that are each other's counterpart and whose bits
    (values > centre) differ in at most max_flip places, the rule that joins windows into a span, are one span heard twice,
    and the more confident of the two is kept (the left one on a tie).  Every other span stays, also where it overlaps a span
    of the other channel: a span is only ever replaced by a counterpart that reads the same payload, so no payload that one
    channel alone would report is dropped, and the result may hold overlapping spans, as a mono scan of two adjacent clips
    does.  In order of their starts."""
    def counterpart(s, others):
        shared = [min(s["end"], o["end"]) - max(s["start"], o["start"]) for o in others]
        return int(np.argmax(shared)) if shared and max(shared) > 0 else None

    def same_payload(a, b):
        return int(np.count_nonzero((np.asarray(a["values"]) > centre) != (np.asarray(b["values"]) > centre))) <= max_flip

    kept, lost = [], set()
    for j, r in enumerate(right):
        i = counterpart(r, left)
        if i is not None and counterpart(left[i], right) == j and same_payload(left[i], r):
            if r["confidence"] > left[i]["confidence"]:
                lost.add(i)
                kept.append(r)
        else:
            kept.append(r)
    kept += [l for i, l in enumerate(left) if i not in lost]
    return sorted(kept, key=lambda k: (k["start"], k["end"]))


def scan_watermark(audio: np.ndarray, sample_rate: int, detector, **options):
    """The marked spans of a long recording (AWAREDetector.scan; options: its keywords window_seconds, hop_samples,
    sync_search, min_confidence, max_flip, max_segments): a list of dicts, in order, of `start`, `end` and `peak` (samples),
    `confidence`, `payload` (the span's values through PatternDecoder) and `values`, and with a payload_code on the detector
    `message`, `valid` and `corrected` of the span's decoded frame (valid informs; it does not filter).  16 kHz only; mono 1-D, or stereo
    [N, 2]: both channels are scanned, and of two spans, one per channel, that are each other's largest overlap and read
    the same payload to within max_flip bits the more confident one is kept (_scan_stereo)."""
    audio = np.asarray(audio)
    if audio.ndim == 2 and audio.shape[1] == 2:
        left, right = _scan(detector, [audio[:, 0], audio[:, 1]], sample_rate, options)
        n_bits = len((left + right)[0]["values"]) if left or right else 0
        flip = options.get("max_flip")
        return _scan_stereo(left, right, n_bits // 4 if flip is None else int(flip), detector._centre())
    if audio.ndim == 1:
        return _scan(detector, [audio], sample_rate, options)[0]
    logger.error("Invalid audio shape. Expected 1D or 2D numpy array.")
    raise ValueError("Invalid audio shape. Expected 1D or 2D numpy array.")


def scan_watermark_batch(files, sample_rate: int, detector, **options):
    """scan_watermark for a list of mono recordings of any lengths, in one scan: a list of span lists."""
    return _scan(detector, files, sample_rate, options)


def _coded(detector):
    if not getattr(detector, "payload_code", None):
        raise ValueError("detect_message: the detector has no payload_code (model card key `payload_code`)")


def _messages(detector, values):
    """decode_messages on rows of values, each result with its `values` row."""
    rows = values.detach().cpu().numpy()
    return [dict(m, values=rows[r]) for r, m in enumerate(detector.decode_messages(values))]


def detect_message(audio: np.ndarray, sample_rate: int, detector, sync_search=None, speed_search=None):
    """EXTENSION: the message of a clip that embed_message marked (the detector's payload_code; utils/watermark/fec.py): the
    existing detection, searches included, then the Viterbi decoder (one aware_viterbi_decode) -> {"message": the k decoded
    bits, "bytes": their first k // 8 bytes, "valid": the CRC's verdict (with a CRC of 0 bits: a finite metric), "corrected":
    the positions the decoder changed, "metric", "values"}.  16 kHz only; mono 1-D, or stereo [N, 2]: both channels are
    decoded and the valid one is kept, of two valid ones (or none) the one with the larger metric, the left one on a tie."""
    if sample_rate != 16000:
        logger.error(f"Invalid sample rate. Expected 16000Hz, got {sample_rate}Hz.")
        raise ValueError("Invalid sample rate. Expected 16000Hz.")
    _coded(detector)
    audio = np.asarray(audio)
    if audio.ndim == 2 and audio.shape[1] == 2:
        l, r = _messages(detector, _detect(detector, [audio[:, 0].astype(np.float32), audio[:, 1].astype(np.float32)],
                                           sample_rate, sync_search, speed_search))
        if l["valid"] != r["valid"]:
            return l if l["valid"] else r
        return r if r["metric"] > l["metric"] else l
    if audio.ndim == 1:
        return _messages(detector, _detect(detector, [audio.astype(np.float32)], sample_rate, sync_search, speed_search))[0]
    logger.error("Invalid audio shape. Expected 1D or 2D numpy array.")
    raise ValueError("Invalid audio shape. Expected 1D or 2D numpy array.")


def detect_message_batch(clips, sample_rate: int, detector, sync_search=None, speed_search=None):
    """detect_message for a list of mono clips of any lengths: one detection, one decode over all clips; a list of dicts."""
    if sample_rate != 16000:
        raise ValueError("Invalid sample rate. Expected 16000Hz.")
    _coded(detector)
    return _messages(detector, _detect(detector, [np.asarray(c, dtype=np.float32) for c in clips], sample_rate, sync_search,
                                       speed_search))
