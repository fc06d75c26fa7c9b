"""`Resample` — `IngestResize` / `ResizeHalf` with a choice of filter: uint8 or float16 RGB frames (0..255 scale) of one size in HBM -> frames
of another, Pillow's two-pass 8-bit resampler with any of its five filters (tables.RESAMPLE_FILTERS: box, bilinear, hamming, bicubic,
lanczos), several frames per launch (include/crtfx_resample.h).  uint8 frames come out byte for byte as `Image.resize((w, h), filter)`
gives them; half frames go through the same arithmetic on quarter codes.  The host builds the two signed integer coefficient tables with
Pillow's float64 expressions (tables.pil_filter_axis); the library copies them."""
from __future__ import annotations

from typing import Tuple

from . import _lib, tables
from ._stage import ResizePlan


class Resample(ResizePlan):
    """plan = Resample(device, (src_h, src_w), (h, w), filter="lanczos", dtype=torch.uint8); out = plan.run(frames[n, src_h, src_w, 3]) ->
    [n, h, w, 3] of the same dtype (torch.uint8 or torch.float16).  `frames` and `out` are tensors on `device` whose frames are contiguous
    (the batch stride is free: slices of larger tensors are fine; half frames must start on an even byte, which every float16 tensor
    does).  The work is enqueued on the current stream of `device`; nothing synchronises.  plan.plan() is crtfx_resample_last_plan as a
    dictionary, e.g. {"resample": "k_resample_fused<u8,rows=16,cols=64>", "lds": "30672", "frames": "5"}."""
    _family = "resample"
    _force_option = _lib.RESAMPLE_OPT_FORCE_GENERAL
    _refusal = "this plan resizes {dtype} frames, got {got}"

    def __init__(self, device, src_size: Tuple[int, int], dst_size: Tuple[int, int], filter: str = "lanczos", dtype=None):     # noqa: A002
        import torch
        if filter not in tables.RESAMPLE_FILTERS:
            raise ValueError(f"filter must be one of {', '.join(tables.RESAMPLE_FILTERS)}, got {filter!r}")
        dtype = torch.uint8 if dtype is None else dtype
        if dtype not in (torch.uint8, torch.float16):
            raise ValueError(f"dtype must be torch.uint8 or torch.float16, got {dtype}")
        self.filter, self.dtype = filter, dtype
        self.itemsize = 1 if dtype == torch.uint8 else 2
        self._dtype = "uint8" if dtype == torch.uint8 else "float16"
        super().__init__(device, src_size, dst_size, _lib.PIX_U8 if dtype == torch.uint8 else _lib.PIX_F16)

    def _axis(self, n_in, n_out):
        return tables.pil_filter_axis(n_in, n_out, self.filter)
