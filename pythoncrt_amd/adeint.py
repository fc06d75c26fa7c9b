"""`AdaptiveDeinterlace` — the motion-adaptive deinterlacer on the device (include/crtfx_adeint.h): where the picture did not change since
the previous source frame the rows a field lacks are the other field's (the weave: full vertical resolution, no bob), where it changed they
are the "edge" interpolation of deint.py, and in between the interpolation is held to within the change of the source's own sample.  It
stands where `Deinterlace` stands and has its orders and field modes; it is causal — the previous source frame is all it needs — so it adds
no latency and the frame count is Deinterlace's.  `run` is the stateless call, `push` the one for a stream of batches (ends.py,
process_frames(deinterlace="adaptive"))."""
from __future__ import annotations

from typing import Tuple

from . import _lib
from ._stage import FramePlan, pix_format
from .deint import FIELDS, ORDERS

METHOD = "adaptive"                 # the value of process_frames(deinterlace=) and --deinterlace that builds this plan; deint.METHODS are Deinterlace's


class AdaptiveDeinterlace(FramePlan):
    """plan = AdaptiveDeinterlace(device, (h, w), order="tff", fields="first", dtype=None);
    out = plan.run(frames[n, h, w, 3], prev=None) -> [n * frames_out, h, w, 3] of the same dtype: source frame i gives output frame i
    ("first") or output frames 2 i and 2 i + 1 ("both").  `prev` is the [h, w, 3] frame in front of frames[0], or None: frames[0] then has no
    previous frame and its output is "edge"'s.  It may be a view of `frames`; it may not overlap `out`.
    plan.push(frames) is run() with the previous frame the plan kept: none at first, then a device copy of the last frame pushed, in a tensor
    the wrapper owns (copied on the current stream behind the kernel, so `frames` may be reused once that stream's work is done);
    plan.reset() forgets it.  The C plan itself keeps nothing.  `dtype` is torch.uint8 (default) or torch.float16.  The work is enqueued on the
    current stream of `device`; nothing synchronises.  plan.plan() is crtfx_adeint_last_plan as a dictionary, e.g.
    {"adeint": "k_adeint<u8,both,vec>", "frames": "5"} (the SOURCE frames of the run)."""
    _family = "adeint"
    _force_option = _lib.ADEINT_OPT_FORCE_GENERAL

    def __init__(self, device, size: Tuple[int, int], order: str = "tff", fields: str = "first", dtype=None, force_general: bool = False):
        for name, value, allowed in (("order", order, ORDERS), ("fields", fields, FIELDS)):
            if value not in allowed:
                raise ValueError(f"{name} must be one of {', '.join(allowed)}, got {value!r}")
        self.order, self.fields = order, fields
        self.frames_out = 2 if fields == "both" else 1
        self._kept, self._has_kept = None, False
        self._open(device)
        self.dtype, pix_fmt = pix_format(dtype)
        self.size = (int(size[0]), int(size[1]))
        self._create(self.size[0], self.size[1], pix_fmt, ORDERS.index(order), FIELDS.index(fields))
        assert self._fn("frames_out")(self._plan) == self.frames_out
        self._frames(self.size + (self.dtype,))
        if force_general:
            self.force_general = True

    def run(self, frames, out=None, prev=None):
        h, w = self.size
        n = self._check_frames(frames)
        if prev is not None and (prev.dtype != self.dtype or tuple(prev.shape) != (h, w, 3) or prev.device != self.device or not prev.is_contiguous()):
            raise ValueError(f"prev must be one contiguous {self.dtype} [{h}, {w}, 3] frame on {self.device}, got {prev.dtype} {tuple(prev.shape)} on {prev.device}")
        return self._run(frames, self._check_out(n, out), n, None if prev is None else prev.data_ptr())

    def push(self, frames, out=None):
        """run() behind the frames pushed before: the previous frame is the last frame of the push before this one (none behind reset() or at
        first).  n = 0 keeps what it had."""
        import torch
        out = self.run(frames, out, self._kept if self._has_kept else None)
        if int(frames.shape[0]):
            if self._kept is None:
                self._kept = torch.empty(self.size + (3,), dtype=self.dtype, device=self.device)
            self._kept.copy_(frames[-1])            # on the current stream, behind the kernel that read the frame kept before
            self._has_kept = True
        return out

    def reset(self) -> None:
        """Forget the kept frame: the next frame pushed has no previous frame (a new stream, a size change, a seek)."""
        self._has_kept = False
