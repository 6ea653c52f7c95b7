from .embed import embed_watermark, embed_watermark_batch, embed_message, embed_message_batch
from .detect import (detect_watermark, detect_watermark_batch, scan_watermark, scan_watermark_batch, detect_message,
                     detect_message_batch)

__all__ = ["embed_watermark", "detect_watermark", "embed_watermark_batch", "detect_watermark_batch", "scan_watermark",
           "scan_watermark_batch", "embed_message", "embed_message_batch", "detect_message", "detect_message_batch"]
