"""`ResizeHalf` — `IngestResize` for a chain that runs on half pixels: float16 RGB frames (0..255 scale) of one size in HBM -> frames of
another, Pillow's two-pass BILINEAR resampler on the quarter-code scale of the 10-bit stages (include/crtfx_resize16.h), several frames per
launch.  The host builds the two integer coefficient tables with Pillow's float64 expressions (tables.pil_resample_axis: the ones
IngestResize hands over); the library copies them."""
from __future__ import annotations

import ctypes
from typing import Tuple

from . import _lib, tables


class ResizeHalf:
    """plan = ResizeHalf(device, (src_h, src_w), (h, w)); out = plan.run(frames_f16[n, src_h, src_w, 3]) -> float16[n, h, w, 3].
    `frames` and `out` are tensors on `device` whose frames are contiguous (the batch stride is free: slices of larger tensors are
    fine).  The work is enqueued on the current stream of `device`; nothing synchronises."""

    def __init__(self, device, src_size: Tuple[int, int], dst_size: Tuple[int, int], pix_fmt: int = _lib.PIX_F16):
        import torch
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"ResizeHalf needs a ROCm device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.src_size = (int(src_size[0]), int(src_size[1]))
        self.dst_size = (int(dst_size[0]), int(dst_size[1]))
        if min(self.src_size + self.dst_size) < 1:
            raise _lib.CrtfxError(_lib.E_INVALID, f"sizes {self.src_size} -> {self.dst_size} must be at least 1 x 1")
        ax = tables.pil_resample_axis(self.src_size[1], self.dst_size[1])
        ay = tables.pil_resample_axis(self.src_size[0], self.dst_size[0])
        self._plan = ctypes.c_void_p()
        rc = self.lib.crtfx_resize16_create(self.device.index, self.src_size[0], self.src_size[1], self.dst_size[0], self.dst_size[1], int(pix_fmt),
                                            tables.ptr(ax[0]), tables.ptr(ax[1]), tables.ptr(ax[2]), ax[2].shape[1],
                                            tables.ptr(ay[0]), tables.ptr(ay[1]), tables.ptr(ay[2]), ay[2].shape[1], ctypes.byref(self._plan))
        if rc != _lib.OK:
            self._plan = None
            raise _lib.CrtfxError(rc, (self.lib.crtfx_resize16_last_error(None) or b"").decode())

    def _check(self, rc):
        if rc != _lib.OK:
            raise _lib.CrtfxError(rc, (self.lib.crtfx_resize16_last_error(self._plan) or b"").decode())

    def set_option(self, option: int, value: int) -> None:
        """Testing / A-B switches (crtfx_resize16_option), e.g. set_option(_lib.RESIZE16_OPT_FORCE_GENERAL, 1)."""
        self._check(self.lib.crtfx_resize16_set_option(self._plan, int(option), int(value)))

    def run(self, frames, out=None):
        import torch
        (sh, sw), (h, w) = self.src_size, self.dst_size
        if frames.dtype != torch.float16:
            raise _lib.CrtfxError(_lib.E_UNSUPPORTED, f"only half RGB frames are resized here, got {frames.dtype} (uint8 frames have IngestResize)")
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (sh, sw, 3) or frames.device != self.device:
            raise ValueError(f"frames must be float16 [n, {sh}, {sw}, 3] on {self.device}, got {tuple(frames.shape)} on {frames.device}")
        n = int(frames.shape[0])
        if out is None:
            out = torch.empty((n, h, w, 3), dtype=torch.float16, device=self.device)
        if out.dtype != torch.float16 or tuple(out.shape) != (n, h, w, 3) or out.device != self.device:
            raise ValueError(f"out must be float16 [{n}, {h}, {w}, 3] on {self.device}")
        for name, t in (("frames", frames), ("out", out)):
            if n and not t[0].is_contiguous():
                raise ValueError(f"every frame of `{name}` must be contiguous (only the batch stride is free)")
        if n == 0:
            return out
        with torch.cuda.device(self.device):
            self._check(self.lib.crtfx_resize16_run(self._plan, frames.data_ptr(), frames.stride(0) * 2, out.data_ptr(), out.stride(0) * 2, n,
                                                    torch.cuda.current_stream(self.device).cuda_stream))
        return out

    def plan(self) -> dict:
        """crtfx_resize16_last_plan as a dictionary, e.g. {"resize16": "k_resize16_fused<rows=32,cols=128>", "lds": "24224", "frames": "5"}."""
        buf = ctypes.create_string_buffer(256)
        self._check(self.lib.crtfx_resize16_last_plan(self._plan, buf, len(buf)))
        return dict(kv.split("=", 1) for kv in buf.value.decode().split(";") if kv)

    def close(self) -> None:
        if getattr(self, "_plan", None):
            self.lib.crtfx_resize16_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 - interpreter shutdown
            pass
