"""`UnpackYuv` — the step in front of the reference's render loop on the device: no decoder produces rgb24 (software decoders hand out
yuv420p, hardware decoders nv12), so every user of the reference's `FFmpegRawReader` (ref:469-514) puts `-pix_fmt rgb24` in front of it and
libswscale converts every source frame on one host core.  Here uint8 yuv420p (I420) or nv12 frames in HBM, 1.5 bytes per pixel, become the
uint8 RGB frames the chain takes, several frames per launch (include/crtfx_unpack.h holds the arithmetic and the two kernel paths).  The
host builds the integer matrix (tables.rgb_matrix); the library copies it.  The mirror image of `EgressYuv`; not byte-equal to libswscale
— see the header."""
from __future__ import annotations

import ctypes
from typing import Tuple

from . import _lib, tables
from .egress import frame_bytes, split_planes  # noqa: F401 - the layout is the egress stage's, read instead of written

LAYOUTS = {"yuv420p": _lib.UNPACK_YUV420P, "nv12": _lib.UNPACK_NV12}


class UnpackYuv:
    """plan = UnpackYuv(device, (h, w), layout="yuv420p", matrix="bt601", range="tv"); rgb = plan.run(packed_u8[n, frame_bytes]) ->
    uint8[n, h, w, 3].  `packed` and `out` are tensors on `device` whose frames are contiguous (the batch stride is free: slices of larger
    tensors are fine).  The work is enqueued on the current stream of `device`; nothing synchronises."""

    def __init__(self, device, size: Tuple[int, int], layout: str = "yuv420p", matrix: str = "bt601", range: str = "tv",    # noqa: A002 - the issue's keyword
                 pix_fmt: int = _lib.PIX_U8):
        import torch
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"UnpackYuv needs a ROCm device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if layout not in LAYOUTS:
            raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, got {layout!r}")
        self.size = (int(size[0]), int(size[1]))
        self.layout, self.matrix, self.range = layout, matrix, range
        if min(self.size) < 1:
            raise _lib.CrtfxError(_lib.E_INVALID, f"size {self.size} must be at least 1 x 1")
        m, off = tables.rgb_matrix(matrix, range)
        self.frame_bytes = frame_bytes(*self.size)
        self._plan = ctypes.c_void_p()
        rc = self.lib.crtfx_unpack_create(self.device.index, self.size[0], self.size[1], int(pix_fmt), LAYOUTS[layout], tables.ptr(m), tables.ptr(off),
                                          ctypes.byref(self._plan))
        if rc != _lib.OK:
            self._plan = None
            raise _lib.CrtfxError(rc, (self.lib.crtfx_unpack_last_error(None) or b"").decode())
        assert self.lib.crtfx_unpack_frame_bytes(self._plan) == self.frame_bytes

    def _check(self, rc):
        if rc != _lib.OK:
            raise _lib.CrtfxError(rc, (self.lib.crtfx_unpack_last_error(self._plan) or b"").decode())

    def set_option(self, option: int, value: int) -> None:
        """Testing / A-B switches (crtfx_unpack_option), e.g. set_option(_lib.UNPACK_OPT_FORCE_GENERAL, 1)."""
        self._check(self.lib.crtfx_unpack_set_option(self._plan, int(option), int(value)))

    def run(self, packed, out=None):
        import torch
        h, w = self.size
        if packed.dtype != torch.uint8:
            raise _lib.CrtfxError(_lib.E_UNSUPPORTED, f"only uint8 yuv420p / nv12 frames are converted, got {packed.dtype}")
        if packed.dim() != 2 or int(packed.shape[1]) != self.frame_bytes or packed.device != self.device:
            raise ValueError(f"packed must be uint8 [n, {self.frame_bytes}] on {self.device}, got {tuple(packed.shape)} on {packed.device}")
        n = int(packed.shape[0])
        if out is None:
            out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w, 3) or out.device != self.device:
            raise ValueError(f"out must be uint8 [{n}, {h}, {w}, 3] on {self.device}")
        for name, t in (("packed", packed), ("out", out)):
            if n and not t[0].is_contiguous():
                raise ValueError(f"every frame of `{name}` must be contiguous (only the batch stride is free)")
        if n == 0:
            return out
        with torch.cuda.device(self.device):
            self._check(self.lib.crtfx_unpack_run(self._plan, packed.data_ptr(), packed.stride(0), out.data_ptr(), out.stride(0), n,
                                                  torch.cuda.current_stream(self.device).cuda_stream))
        return out

    def planes(self, packed):
        """Views of `packed` ([n, frame_bytes] or [frame_bytes]; a tensor or a numpy array): (Y, U, V) or (Y, UV) — see egress.split_planes."""
        return split_planes(packed, self.size, self.layout)

    def plan(self) -> dict:
        """crtfx_unpack_last_plan as a dictionary, e.g. {"unpack": "k_unpack_420<nv12,vec>", "frames": "5"}."""
        buf = ctypes.create_string_buffer(256)
        self._check(self.lib.crtfx_unpack_last_plan(self._plan, buf, len(buf)))
        return dict(kv.split("=", 1) for kv in buf.value.decode().split(";") if kv)

    def close(self) -> None:
        if getattr(self, "_plan", None):
            self.lib.crtfx_unpack_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 - interpreter shutdown
            pass
