"""`Lut3D` — `lut3d=` on the device: RGB frames in HBM go through a colour cube with tetrahedral interpolation (include/crtfx_lut3d.h),
several frames per launch.  uint8 frames index the cube with their codes, half frames with their quarter codes; entries and results are
quarter codes 0..1020, so a cube's precision here is 10 bits.  The cube is a `Cube` (pythoncrt_amd/cube.py: what a `.cube` file holds) or
a path to one.  It stands directly in front of the chain and directly behind it (ends.py, process_frames(in_lut=, deliver_lut=))."""
from __future__ import annotations

import ctypes
from typing import Tuple

import numpy as np

from . import _lib
from ._stage import FramePlan, pix_format
from .cube import Cube, as_cube


class Lut3D(FramePlan):
    """plan = Lut3D(device, (h, w), cube, dtype=torch.uint8); out = plan.run(frames[n, h, w, 3]) -> the same dtype and shape (plan(frames)
    is the same call).  `frames` and `out` are tensors on `device` whose frames are contiguous (the batch stride is free: slices of larger
    tensors are fine) and do not overlap.  The work is enqueued on the current stream of `device`; only creating the plan and set_cube
    synchronise.  plan.plan() is crtfx_lut3d_last_plan as a dictionary, e.g. {"lut3d": "k_lut3d<u8,lds,vec>", "n": "33", "lds": "143748",
    "frames": "5"}."""
    _family = "lut3d"
    _force_option = _lib.LUT3D_OPT_FORCE_GENERAL

    def __init__(self, device, size: Tuple[int, int], cube, dtype=None, force_general: bool = False):
        self.dtype, pix_fmt = pix_format(dtype)
        self.cube = cube = as_cube(cube)
        self._open(device)
        self.size = (int(size[0]), int(size[1]))
        table = self._table(cube)
        self._create(self.size[0], self.size[1], pix_fmt, cube.size, table.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)))
        self._frames(self.size + (self.dtype,))
        self._force_global = False
        if force_general:
            self.force_general = True

    @staticmethod
    def _table(cube: Cube) -> np.ndarray:
        return np.ascontiguousarray(cube.quantise(), dtype=np.uint16)

    def set_cube(self, cube) -> None:
        """Swap the cube of the live plan for another of the same size (crtfx_lut3d_set_table; synchronises)."""
        cube = as_cube(cube)
        table = self._table(cube)
        import torch
        with torch.cuda.device(self.device):
            self._check(self._fn("set_table")(self._plan, cube.size, table.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))))
        self.cube = cube

    @property
    def force_global(self) -> bool:
        """Gather from the device table whatever the cube's size (CRTFX_LUT3D_OPT_FORCE_GLOBAL)."""
        return self._force_global

    @force_global.setter
    def force_global(self, value) -> None:
        self.set_option(_lib.LUT3D_OPT_FORCE_GLOBAL, 1 if value else 0)
        self._force_global = bool(value)
