"""`Resample` — `IngestResize` / `ResizeHalf` with a choice of filter: uint8 or float16 RGB frames (0..255 scale) of one size in HBM -> frames
of another, Pillow's two-pass 8-bit resampler with any of its five filters (tables.RESAMPLE_FILTERS: box, bilinear, hamming, bicubic,
lanczos), several frames per launch (include/crtfx_resample.h).  uint8 frames come out byte for byte as `Image.resize((w, h), filter)`
gives them; half frames go through the same arithmetic on quarter codes.  The host builds the two signed integer coefficient tables with
Pillow's float64 expressions (tables.pil_filter_axis); the library copies them."""
from __future__ import annotations

import ctypes
from typing import Tuple

from . import _lib, tables


class Resample:
    """plan = Resample(device, (src_h, src_w), (h, w), filter="lanczos", dtype=torch.uint8); out = plan.run(frames[n, src_h, src_w, 3]) ->
    [n, h, w, 3] of the same dtype (torch.uint8 or torch.float16).  `frames` and `out` are tensors on `device` whose frames are contiguous
    (the batch stride is free: slices of larger tensors are fine; half frames must start on an even byte, which every float16 tensor
    does).  The work is enqueued on the current stream of `device`; nothing synchronises."""

    def __init__(self, device, src_size: Tuple[int, int], dst_size: Tuple[int, int], filter: str = "lanczos", dtype=None):
        import torch
        if filter not in tables.RESAMPLE_FILTERS:
            raise ValueError(f"filter must be one of {', '.join(tables.RESAMPLE_FILTERS)}, got {filter!r}")
        dtype = torch.uint8 if dtype is None else dtype
        if dtype not in (torch.uint8, torch.float16):
            raise ValueError(f"dtype must be torch.uint8 or torch.float16, got {dtype}")
        self.filter, self.dtype = filter, dtype
        self.itemsize = 1 if dtype == torch.uint8 else 2
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"Resample needs a ROCm device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.src_size = (int(src_size[0]), int(src_size[1]))
        self.dst_size = (int(dst_size[0]), int(dst_size[1]))
        if min(self.src_size + self.dst_size) < 1:
            raise _lib.CrtfxError(_lib.E_INVALID, f"sizes {self.src_size} -> {self.dst_size} must be at least 1 x 1")
        ax = tables.pil_filter_axis(self.src_size[1], self.dst_size[1], filter)
        ay = tables.pil_filter_axis(self.src_size[0], self.dst_size[0], filter)
        self._plan = ctypes.c_void_p()
        rc = self.lib.crtfx_resample_create(self.device.index, self.src_size[0], self.src_size[1], self.dst_size[0], self.dst_size[1],
                                            _lib.PIX_U8 if dtype == torch.uint8 else _lib.PIX_F16,
                                            tables.ptr(ax[0]), tables.ptr(ax[1]), tables.ptr(ax[2]), ax[2].shape[1],
                                            tables.ptr(ay[0]), tables.ptr(ay[1]), tables.ptr(ay[2]), ay[2].shape[1], ctypes.byref(self._plan))
        if rc != _lib.OK:
            self._plan = None
            raise _lib.CrtfxError(rc, (self.lib.crtfx_resample_last_error(None) or b"").decode())

    def _check(self, rc):
        if rc != _lib.OK:
            raise _lib.CrtfxError(rc, (self.lib.crtfx_resample_last_error(self._plan) or b"").decode())

    def set_option(self, option: int, value: int) -> None:
        """Testing / A-B switches (crtfx_resample_option), e.g. set_option(_lib.RESAMPLE_OPT_FORCE_GENERAL, 1)."""
        self._check(self.lib.crtfx_resample_set_option(self._plan, int(option), int(value)))

    def run(self, frames, out=None):
        import torch
        (sh, sw), (h, w) = self.src_size, self.dst_size
        if frames.dtype != self.dtype:
            raise _lib.CrtfxError(_lib.E_UNSUPPORTED, f"this plan resizes {self.dtype} frames, got {frames.dtype}")
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (sh, sw, 3) or frames.device != self.device:
            raise ValueError(f"frames must be {self.dtype} [n, {sh}, {sw}, 3] on {self.device}, got {tuple(frames.shape)} on {frames.device}")
        n = int(frames.shape[0])
        if out is None:
            out = torch.empty((n, h, w, 3), dtype=self.dtype, device=self.device)
        if out.dtype != self.dtype or tuple(out.shape) != (n, h, w, 3) or out.device != self.device:
            raise ValueError(f"out must be {self.dtype} [{n}, {h}, {w}, 3] on {self.device}")
        for name, t in (("frames", frames), ("out", out)):
            if n and not t[0].is_contiguous():
                raise ValueError(f"every frame of `{name}` must be contiguous (only the batch stride is free)")
        if n == 0:
            return out
        with torch.cuda.device(self.device):
            self._check(self.lib.crtfx_resample_run(self._plan, frames.data_ptr(), frames.stride(0) * self.itemsize, out.data_ptr(),
                                                    out.stride(0) * self.itemsize, n, torch.cuda.current_stream(self.device).cuda_stream))
        return out

    def plan(self) -> dict:
        """crtfx_resample_last_plan as a dictionary, e.g. {"resample": "k_resample_fused<u8,rows=16,cols=64>", "lds": "30672", "frames": "5"}."""
        buf = ctypes.create_string_buffer(256)
        self._check(self.lib.crtfx_resample_last_plan(self._plan, buf, len(buf)))
        return dict(kv.split("=", 1) for kv in buf.value.decode().split(";") if kv)

    def close(self) -> None:
        if getattr(self, "_plan", None):
            self.lib.crtfx_resample_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 - interpreter shutdown
            pass
