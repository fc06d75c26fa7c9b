"""`ResizeHalf` — `IngestResize` for a chain that runs on half pixels: float16 RGB frames (0..255 scale) of one size in HBM -> frames of
another, Pillow's two-pass BILINEAR resampler on the quarter-code scale of the 10-bit stages (include/crtfx_resize16.h), several frames per
launch.  The host builds the two integer coefficient tables with Pillow's float64 expressions (tables.pil_resample_axis: the ones
IngestResize hands over); the library copies them."""
from __future__ import annotations

from typing import Tuple

from . import _lib
from ._stage import ResizePlan


class ResizeHalf(ResizePlan):
    """plan = ResizeHalf(device, (src_h, src_w), (h, w)); out = plan.run(frames_f16[n, src_h, src_w, 3]) -> float16[n, h, w, 3].
    `frames` and `out` are tensors on `device` whose frames are contiguous (the batch stride is free: slices of larger tensors are
    fine).  The work is enqueued on the current stream of `device`; nothing synchronises.  plan.plan() is crtfx_resize16_last_plan as a
    dictionary, e.g. {"resize16": "k_resize16_fused<rows=32,cols=128>", "lds": "24224", "frames": "5"}."""
    _family = "resize16"
    _force_option = _lib.RESIZE16_OPT_FORCE_GENERAL
    _dtype = "float16"
    _refusal = "only half RGB frames are resized here, got {got} (uint8 frames have IngestResize)"

    def __init__(self, device, src_size: Tuple[int, int], dst_size: Tuple[int, int], pix_fmt: int = _lib.PIX_F16):
        super().__init__(device, src_size, dst_size, pix_fmt)
