"""`IngestResize` — the first step of the reference's render loop, `Image.fromarray(frame).resize((out_w, out_h), Image.BILINEAR)`
(crt_filter.py ref:1039-1041), on the device: uint8 RGB frames of one size in HBM -> frames of another, byte for byte what Pillow's
8-bit resampler produces, several frames per launch (include/crtfx_ingest.h).  The host builds the two integer coefficient tables with
Pillow's float64 expressions (tables.pil_resample_axis); the library copies them."""
from __future__ import annotations

from typing import Tuple

from . import _lib
from ._stage import ResizePlan


class IngestResize(ResizePlan):
    """plan = IngestResize(device, (src_h, src_w), (h, w)); out = plan.run(frames_u8[n, src_h, src_w, 3]) -> uint8[n, h, w, 3].
    `frames` and `out` are tensors on `device` whose frames are contiguous (the batch stride is free: slices of larger tensors are
    fine).  The work is enqueued on the current stream of `device`; nothing synchronises.  plan.plan() is crtfx_ingest_last_plan as a
    dictionary, e.g. {"ingest": "k_ingest_fused<rows=32,cols=128>", "lds": "11880", "frames": "5"}."""
    _family = "ingest"
    _force_option = _lib.INGEST_OPT_FORCE_GENERAL
    _dtype = "uint8"
    _refusal = "only uint8 RGB frames are resized (Pillow has no {got} image)"

    def __init__(self, device, src_size: Tuple[int, int], dst_size: Tuple[int, int], pix_fmt: int = _lib.PIX_U8):
        super().__init__(device, src_size, dst_size, pix_fmt)
