"""Watermark pattern codec (bits / bytes <-> bipolar), and the channel code of coded payloads (fec)."""
from . import fec  # noqa: F401
from .codec import PatternDecoder, PatternEncoder  # noqa: F401

__all__ = ("PatternEncoder", "PatternDecoder", "fec")
