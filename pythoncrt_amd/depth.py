"""`Widen` and `Narrow` — `format=` on the device: RGB frames in HBM change their sample type (include/crtfx_depth.h), several frames per
launch.  `Widen` turns uint8 frames into float16 frames of the same codes, exactly; `Narrow` turns finished float16 frames into uint8 ones,
rounding to nearest (ties to even, as the uint8 chain's own quantiser does) or with an 8 x 8 ordered dither whose thresholds are
(2 * BAYER8 + 1) / 128.  With them the two ends of a render need not have the same depth (ends.py, process_frames(chain_pix="half"))."""
from __future__ import annotations

from typing import Tuple

from . import _lib
from ._stage import FramePlan

DITHERS = ("none", "ordered")

# B[y][x] of include/crtfx_depth.h (CRTFX_DEPTH_BAYER8): the index matrix of the recursive 2 x 2 construction
BAYER8 = ((0, 32, 8, 40, 2, 34, 10, 42),
          (48, 16, 56, 24, 50, 18, 58, 26),
          (12, 44, 4, 36, 14, 46, 6, 38),
          (60, 28, 52, 20, 62, 30, 54, 22),
          (3, 35, 11, 43, 1, 33, 9, 41),
          (51, 19, 59, 27, 49, 17, 57, 25),
          (15, 47, 7, 39, 13, 45, 5, 37),
          (63, 31, 55, 23, 61, 29, 53, 21))


class _Depth(FramePlan):
    """What the two directions share: out = plan.run(frames[n, h, w, 3] of `_src`) -> [n, h, w, 3] of `_dst` (plan(frames) is the same
    call).  `frames` and `out` are tensors on `device` whose frames are contiguous (the batch stride is free: slices of larger tensors are
    fine).  The work is enqueued on the current stream of `device`; nothing synchronises."""
    _family = "depth"
    _force_option = _lib.DEPTH_OPT_FORCE_GENERAL
    _direction = _lib.DEPTH_WIDEN
    _src, _dst = "uint8", "float16"

    def _plan_for(self, device, size, dither, force_general):
        import torch
        self._open(device)
        self.size = (int(size[0]), int(size[1]))
        self._create(self.size[0], self.size[1], self._direction, dither)
        self._frames(self.size + (getattr(torch, self._src),), self.size + (getattr(torch, self._dst),))
        if force_general:
            self.force_general = True


class Widen(_Depth):
    """plan = Widen(device, (h, w)); out = plan.run(frames_u8[n, h, w, 3]) -> float16 [n, h, w, 3]: half(u), exact.  plan.plan() is
    crtfx_depth_last_plan as a dictionary, e.g. {"depth": "k_widen<vec>", "frames": "5"}."""

    def __init__(self, device, size: Tuple[int, int], force_general: bool = False):
        self._plan_for(device, size, _lib.DITHER_NONE, force_general)


class Narrow(_Depth):
    """plan = Narrow(device, (h, w), dither="none"); out = plan.run(frames_f16[n, h, w, 3]) -> uint8 [n, h, w, 3]: the half clamped to
    0..255 (NaN -> 0), then rounded to nearest, ties to even ("none"), or floor(v + t[y & 7][x & 7]) with t = (2 * BAYER8 + 1) / 128
    ("ordered": one threshold per pixel, at the pixel's place in the frame given).  plan.plan() is e.g.
    {"depth": "k_narrow<ordered,vec>", "frames": "5"}."""
    _direction = _lib.DEPTH_NARROW
    _src, _dst = "float16", "uint8"

    def __init__(self, device, size: Tuple[int, int], dither: str = "none", force_general: bool = False):
        if dither not in DITHERS:
            raise ValueError(f"dither must be one of {', '.join(DITHERS)}, got {dither!r}")
        self.dither = dither
        self._plan_for(device, size, _lib.DITHER_ORDERED if dither == "ordered" else _lib.DITHER_NONE, force_general)
