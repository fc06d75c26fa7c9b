"""`Lut3D` — `lut3d=` on the device: RGB frames in HBM go through a colour cube with tetrahedral interpolation (include/crtfx_lut3d.h),
several frames per launch.  uint8 frames index the cube with their codes, half frames with their quarter codes; entries and results are
quarter codes 0..1020, so a cube's precision here is 10 bits.  The cube is a `Cube` (pythoncrt_amd/cube.py: what a `.cube` file holds) or
a path to one.  It stands directly in front of the chain and directly behind it (ends.py, process_frames(in_lut=, deliver_lut=))."""
from __future__ import annotations

import ctypes
from typing import Tuple

import numpy as np

from . import _lib
from ._stage import Handle
from .cube import Cube, as_cube


class Lut3D(Handle):
    """plan = Lut3D(device, (h, w), cube, dtype=torch.uint8); out = plan.run(frames[n, h, w, 3]) -> the same dtype and shape (plan(frames)
    is the same call).  `frames` and `out` are tensors on `device` whose frames are contiguous (the batch stride is free: slices of larger
    tensors are fine) and do not overlap.  The work is enqueued on the current stream of `device`; only creating the plan and set_cube
    synchronise.  plan.plan() is crtfx_lut3d_last_plan as a dictionary, e.g. {"lut3d": "k_lut3d<u8,lds,vec>", "n": "33", "lds": "143748",
    "frames": "5"}."""
    _family = "lut3d"
    _force_option = _lib.LUT3D_OPT_FORCE_GENERAL

    def __init__(self, device, size: Tuple[int, int], cube, dtype=None, force_general: bool = False):
        import torch
        dtype = torch.uint8 if dtype is None else dtype
        if dtype not in (torch.uint8, torch.float16):
            raise ValueError(f"dtype must be torch.uint8 or torch.float16, got {dtype}")
        cube = as_cube(cube)
        self._open(device)
        self.size = (int(size[0]), int(size[1]))
        self.dtype, self.cube = dtype, cube
        table = self._table(cube)
        self._create(self.size[0], self.size[1], _lib.PIX_F16 if dtype == torch.float16 else _lib.PIX_U8, cube.size,
                     table.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)))
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

    def run(self, frames, out=None):
        import torch
        h, w = self.size
        if frames.dtype != self.dtype:
            raise _lib.CrtfxError(_lib.E_UNSUPPORTED, f"this plan takes {self.dtype} RGB frames, got {frames.dtype}")
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (h, w, 3) or frames.device != self.device:
            raise ValueError(f"frames must be {self.dtype} [n, {h}, {w}, 3] on {self.device}, got {tuple(frames.shape)} on {frames.device}")
        n = int(frames.shape[0])
        if out is None:
            out = torch.empty((n, h, w, 3), dtype=self.dtype, device=self.device)
        if out.dtype != self.dtype or tuple(out.shape) != (n, h, w, 3) or out.device != self.device:
            raise ValueError(f"out must be {self.dtype} [{n}, {h}, {w}, 3] on {self.device}")
        return self._run(frames, out, n)
