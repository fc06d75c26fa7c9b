"""`Interlace` — `interlace` / `tinterlace`'s place on the device, the delivery pair of the deinterlacers: two consecutive finished RGB
frames in HBM — the two fields of a chain that runs at field rate — are woven into one interlaced frame (include/crtfx_interlace.h),
several frames per launch.  Row y of an output frame is row y of the first frame of its pair where y has the first field's parity, of the
second frame elsewhere; `lowpass` filters each row vertically inside ITS frame before the weave, against line twitter: "linear" is
[1 2 1] / 4, "complex" [-1 2 6 2 -1] / 8 held back from over-sharpening.  It stands behind the delivery resize and the Canvas and in front
of the Narrow and the egress plan (ends.py, process_frames(deliver_interlace=))."""
from __future__ import annotations

from typing import Tuple

from . import _lib
from ._stage import FramePlan, pix_format

ORDERS = ("tff", "bff")
LOWPASS = ("none", "linear", "complex")


class Interlace(FramePlan):
    """plan = Interlace(device, (h, w), order="tff", lowpass="none", dtype=None);
    out = plan.run(frames[n, h, w, 3]) -> [ceil(n / 2), h, w, 3] of the same dtype (plan(frames) is the same call): output frame j is woven
    from source frames 2 j and min(2 j + 1, n - 1), so an odd last frame is woven with itself.  `dtype` is torch.uint8 (default) or
    torch.float16.  `frames` and `out` are tensors on `device` whose frames are contiguous (the batch stride is free: slices of larger
    tensors are fine).  The work is enqueued on the current stream of `device`; nothing synchronises.  plan.plan() is
    crtfx_interlace_last_plan as a dictionary, e.g. {"interlace": "k_interlace<linear,u8,vec>", "frames": "6"} (the SOURCE frames of the
    run).  The chroma rows of a 4:2:0 delivery are formed behind this stage: by the family's egress plan and EgressSited as a progressive
    frame's are, so they mix the two fields, or by EgressField420 (out_chroma_rows="interlaced") from rows of their own field only; 4:2:2,
    4:4:4 and rgb24 deliveries have no such pairing."""
    _family = "interlace"
    _force_option = _lib.INTERLACE_OPT_FORCE_GENERAL
    frames_in = 2

    def __init__(self, device, size: Tuple[int, int], order: str = "tff", lowpass: str = "none", dtype=None, force_general: bool = False):
        for name, value, allowed in (("order", order, ORDERS), ("lowpass", lowpass, LOWPASS)):
            if value not in allowed:
                raise ValueError(f"{name} must be one of {', '.join(allowed)}, got {value!r}")
        self.order, self.lowpass = order, lowpass
        self._open(device)
        self.dtype, pix_fmt = pix_format(dtype)
        self.size = (int(size[0]), int(size[1]))
        self._create(self.size[0], self.size[1], pix_fmt, ORDERS.index(order), LOWPASS.index(lowpass))
        assert self._fn("frames_in")(self._plan) == self.frames_in
        self._frames(self.size + (self.dtype,))
        if force_general:
            self.force_general = True
