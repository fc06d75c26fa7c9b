"""`AdaptiveDeinterlace` — the motion-adaptive deinterlacer on the device (include/crtfx_adeint.h): where the picture did not change since
the previous source frame the rows a field lacks are the other field's (the weave: full vertical resolution, no bob), where it changed they
are the "edge" interpolation of deint.py, and in between the interpolation is held to within the change of the source's own sample.  It
stands where `Deinterlace` stands and has its orders and field modes; it is causal — the previous source frame is all it needs — so it adds
no latency and the frame count is Deinterlace's.  `run` is the stateless call, `push` the one for a stream of batches (ends.py,
process_frames(deinterlace="adaptive"))."""
from __future__ import annotations

from typing import Tuple

from . import _lib
from ._stage import Handle
from .deint import FIELDS, ORDERS

METHOD = "adaptive"                 # the value of process_frames(deinterlace=) and --deinterlace that builds this plan; deint.METHODS are Deinterlace's


class AdaptiveDeinterlace(Handle):
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
        import torch
        self.dtype = torch.uint8 if dtype is None else dtype
        if self.dtype not in (torch.uint8, torch.float16):
            raise ValueError(f"dtype must be torch.uint8 or torch.float16, got {dtype!r}")
        self.size = (int(size[0]), int(size[1]))
        self._create(self.size[0], self.size[1], _lib.PIX_F16 if self.dtype == torch.float16 else _lib.PIX_U8, ORDERS.index(order), FIELDS.index(fields))
        assert self._fn("frames_out")(self._plan) == self.frames_out
        if force_general:
            self.force_general = True

    def run(self, frames, out=None, prev=None):
        import torch
        h, w = self.size
        if frames.dtype != self.dtype:
            raise _lib.CrtfxError(_lib.E_UNSUPPORTED, f"this plan takes {self.dtype} RGB frames, got {frames.dtype}")
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (h, w, 3) or frames.device != self.device:
            raise ValueError(f"frames must be {self.dtype} [n, {h}, {w}, 3] on {self.device}, got {tuple(frames.shape)} on {frames.device}")
        if prev is not None and (prev.dtype != self.dtype or tuple(prev.shape) != (h, w, 3) or prev.device != self.device or not prev.is_contiguous()):
            raise ValueError(f"prev must be one contiguous {self.dtype} [{h}, {w}, 3] frame on {self.device}, got {prev.dtype} {tuple(prev.shape)} on {prev.device}")
        n = int(frames.shape[0])
        if out is None:
            out = torch.empty((n * self.frames_out, h, w, 3), dtype=self.dtype, device=self.device)
        if out.dtype != self.dtype or tuple(out.shape) != (n * self.frames_out, h, w, 3) or out.device != self.device:
            raise ValueError(f"out must be {self.dtype} [{n * self.frames_out}, {h}, {w}, 3] on {self.device}")
        for name, t in (("input", frames), ("out", out)):
            if n and not t[0].is_contiguous():
                raise ValueError(f"every frame of the {name} must be contiguous (only the batch stride is free)")
        if n == 0:
            return out
        with torch.cuda.device(self.device):
            self._check(self._fn("run")(self._plan, None if prev is None else prev.data_ptr(), frames.data_ptr(), frames.stride(0) * frames.element_size(),
                                        out.data_ptr(), out.stride(0) * out.element_size(), n, torch.cuda.current_stream(self.device).cuda_stream))
        return out

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
