"""`IngestResize` — the first step of the reference's render loop, `Image.fromarray(frame).resize((out_w, out_h), Image.BILINEAR)`
(crt_filter.py ref:1039-1041), on the device: uint8 RGB frames of one size in HBM -> frames of another, byte for byte what Pillow's
8-bit resampler produces, several frames per launch (include/crtfx_ingest.h).  The host builds the two integer coefficient tables with
Pillow's float64 expressions (tables.pil_resample_axis); the library copies them."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

from . import _lib, tables


class IngestResize:
    """plan = IngestResize(device, (src_h, src_w), (h, w)); out = plan.run(frames_u8[n, src_h, src_w, 3]) -> uint8[n, h, w, 3].
    `frames` and `out` are tensors on `device` whose frames are contiguous (the batch stride is free: slices of larger tensors are
    fine).  The work is enqueued on the current stream of `device`; nothing synchronises."""

    def __init__(self, device, src_size: Tuple[int, int], dst_size: Tuple[int, int], pix_fmt: int = _lib.PIX_U8):
        import torch
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"IngestResize needs a ROCm device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.src_size = (int(src_size[0]), int(src_size[1]))
        self.dst_size = (int(dst_size[0]), int(dst_size[1]))
        if min(self.src_size + self.dst_size) < 1:
            raise _lib.CrtfxError(_lib.E_INVALID, f"sizes {self.src_size} -> {self.dst_size} must be at least 1 x 1")
        ax = tables.pil_resample_axis(self.src_size[1], self.dst_size[1])
        ay = tables.pil_resample_axis(self.src_size[0], self.dst_size[0])
        self._plan = ctypes.c_void_p()
        rc = self.lib.crtfx_ingest_create(self.device.index, self.src_size[0], self.src_size[1], self.dst_size[0], self.dst_size[1], int(pix_fmt),
                                          tables.ptr(ax[0]), tables.ptr(ax[1]), tables.ptr(ax[2]), ax[2].shape[1],
                                          tables.ptr(ay[0]), tables.ptr(ay[1]), tables.ptr(ay[2]), ay[2].shape[1], ctypes.byref(self._plan))
        if rc != _lib.OK:
            self._plan = None
            raise _lib.CrtfxError(rc, (self.lib.crtfx_ingest_last_error(None) or b"").decode())

    def _check(self, rc):
        if rc != _lib.OK:
            raise _lib.CrtfxError(rc, (self.lib.crtfx_ingest_last_error(self._plan) or b"").decode())

    def set_option(self, option: int, value: int) -> None:
        """Testing / A-B switches (crtfx_ingest_option), e.g. set_option(_lib.INGEST_OPT_FORCE_GENERAL, 1)."""
        self._check(self.lib.crtfx_ingest_set_option(self._plan, int(option), int(value)))

    def run(self, frames, out=None):
        import torch
        (sh, sw), (h, w) = self.src_size, self.dst_size
        if frames.dtype != torch.uint8:
            raise _lib.CrtfxError(_lib.E_UNSUPPORTED, f"only uint8 RGB frames are resized (Pillow has no {frames.dtype} image)")
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (sh, sw, 3) or frames.device != self.device:
            raise ValueError(f"frames must be uint8 [n, {sh}, {sw}, 3] on {self.device}, got {tuple(frames.shape)} on {frames.device}")
        n = int(frames.shape[0])
        if out is None:
            out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w, 3) or out.device != self.device:
            raise ValueError(f"out must be uint8 [{n}, {h}, {w}, 3] on {self.device}")
        for name, t in (("frames", frames), ("out", out)):
            if n and not t[0].is_contiguous():
                raise ValueError(f"every frame of `{name}` must be contiguous (only the batch stride is free)")
        if n == 0:
            return out
        with torch.cuda.device(self.device):
            self._check(self.lib.crtfx_ingest_run(self._plan, frames.data_ptr(), frames.stride(0), out.data_ptr(), out.stride(0), n,
                                                  torch.cuda.current_stream(self.device).cuda_stream))
        return out

    def plan(self) -> dict:
        """crtfx_ingest_last_plan as a dictionary, e.g. {"ingest": "k_ingest_fused<rows=32,cols=128>", "lds": "11880", "frames": "5"}."""
        buf = ctypes.create_string_buffer(256)
        self._check(self.lib.crtfx_ingest_last_plan(self._plan, buf, len(buf)))
        return dict(kv.split("=", 1) for kv in buf.value.decode().split(";") if kv)

    def close(self) -> None:
        if getattr(self, "_plan", None):
            self.lib.crtfx_ingest_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 - interpreter shutdown
            pass
