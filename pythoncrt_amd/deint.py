"""`Deinterlace` — `yadif`'s place on the device: RGB frames in HBM that carry two fields woven into their even and odd rows become
progressive frames (include/crtfx_deint.h), several frames per launch.  The rows of a field are kept as bits; the rows between them are
interpolated from the kept rows above and below, straight down ("linear") or along the best of five directions per pixel ("edge").
`fields="first"` gives one frame per source frame, `"both"` one per field, in field order: the chain behind it then runs at field rate
(ends.py, process_frames(deinterlace=))."""
from __future__ import annotations

from typing import Tuple

from . import _lib
from ._stage import FramePlan, pix_format

METHODS = ("linear", "edge")
ORDERS = ("tff", "bff")
FIELDS = ("first", "both")


class Deinterlace(FramePlan):
    """plan = Deinterlace(device, (h, w), method="linear", order="tff", fields="first", dtype=None);
    out = plan.run(frames[n, h, w, 3]) -> [n * frames_out, h, w, 3] of the same dtype (plan(frames) is the same call): source frame i
    gives output frame i ("first") or output frames 2 i and 2 i + 1 ("both").  `dtype` is torch.uint8 (default) or torch.float16.
    `frames` and `out` are tensors on `device` whose frames are contiguous (the batch stride is free: slices of larger tensors are fine).
    The work is enqueued on the current stream of `device`; nothing synchronises.  plan.plan() is crtfx_deint_last_plan as a dictionary,
    e.g. {"deint": "k_deint<edge,u8,both,vec>", "frames": "5"} (the SOURCE frames of the run)."""
    _family = "deint"
    _force_option = _lib.DEINT_OPT_FORCE_GENERAL

    def __init__(self, device, size: Tuple[int, int], method: str = "linear", order: str = "tff", fields: str = "first", dtype=None,
                 force_general: bool = False):
        for name, value, allowed in (("method", method, METHODS), ("order", order, ORDERS), ("fields", fields, FIELDS)):
            if value not in allowed:
                raise ValueError(f"{name} must be one of {', '.join(allowed)}, got {value!r}")
        self.method, self.order, self.fields = method, order, fields
        self.frames_out = 2 if fields == "both" else 1
        self._open(device)
        self.dtype, pix_fmt = pix_format(dtype)
        self.size = (int(size[0]), int(size[1]))
        self._create(self.size[0], self.size[1], pix_fmt, METHODS.index(method), ORDERS.index(order), FIELDS.index(fields))
        assert self._fn("frames_out")(self._plan) == self.frames_out
        self._frames(self.size + (self.dtype,))
        if force_general:
            self.force_general = True
