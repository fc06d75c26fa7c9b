"""`EgressYuv` — the last step of the reference's render loop on the device: each of its encoder branches ends in `-pix_fmt yuv420p`
(crt_filter.py ref:970-1002), so every finished rgb24 frame is converted to 4:2:0 by libswscale on one host core.  Here finished uint8 RGB
frames in HBM become yuv420p (I420) or nv12 frames of 1.5 bytes per pixel, several frames per launch (include/crtfx_egress.h holds the
arithmetic and the two kernel paths).  The host builds the integer matrix (tables.yuv_matrix); the library copies it.  Not byte-equal to
libswscale — see the header."""
from __future__ import annotations

import ctypes
from typing import Tuple

from . import _lib, tables

LAYOUTS = {"yuv420p": _lib.EGRESS_YUV420P, "nv12": _lib.EGRESS_NV12}


def frame_bytes(h: int, w: int) -> int:
    """Bytes of one h x w yuv420p / nv12 frame: h * w + 2 * ceil(h / 2) * ceil(w / 2)."""
    return int(h) * int(w) + 2 * ((int(h) + 1) // 2) * ((int(w) + 1) // 2)


def split_planes(out, size: Tuple[int, int], layout: str):
    """Views of `out` ([..., frame_bytes]; a tensor or a numpy array) for an h x w frame: (Y [.., h, w], U [.., ch, cw], V [.., ch, cw])
    for yuv420p, (Y, UV [.., ch, cw, 2]) for nv12, with ch = ceil(h / 2) and cw = ceil(w / 2)."""
    h, w = int(size[0]), int(size[1])
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, got {layout!r}")
    lead = tuple(out.shape[:-1])
    if int(out.shape[-1]) != frame_bytes(h, w):
        raise ValueError(f"the last axis must hold {frame_bytes(h, w)} bytes, got {tuple(out.shape)}")
    y = out[..., :h * w].reshape(lead + (h, w))
    if layout == "nv12":
        return y, out[..., h * w:].reshape(lead + (ch, cw, 2))
    return y, out[..., h * w:h * w + ch * cw].reshape(lead + (ch, cw)), out[..., h * w + ch * cw:].reshape(lead + (ch, cw))


class EgressYuv:
    """plan = EgressYuv(device, (h, w), layout="yuv420p", matrix="bt601", range="tv"); out = plan.run(frames_u8[n, h, w, 3]) ->
    uint8[n, frame_bytes].  `frames` and `out` are tensors on `device` whose frames are contiguous (the batch stride is free: slices of
    larger tensors are fine).  The work is enqueued on the current stream of `device`; nothing synchronises."""

    def __init__(self, device, size: Tuple[int, int], layout: str = "yuv420p", matrix: str = "bt601", range: str = "tv",    # noqa: A002 - the issue's keyword
                 pix_fmt: int = _lib.PIX_U8):
        import torch
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"EgressYuv needs a ROCm device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if layout not in LAYOUTS:
            raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, got {layout!r}")
        self.size = (int(size[0]), int(size[1]))
        self.layout, self.matrix, self.range = layout, matrix, range
        if min(self.size) < 1:
            raise _lib.CrtfxError(_lib.E_INVALID, f"size {self.size} must be at least 1 x 1")
        m, off = tables.yuv_matrix(matrix, range)
        self.frame_bytes = frame_bytes(*self.size)
        self._plan = ctypes.c_void_p()
        rc = self.lib.crtfx_egress_create(self.device.index, self.size[0], self.size[1], int(pix_fmt), LAYOUTS[layout], tables.ptr(m), tables.ptr(off),
                                          ctypes.byref(self._plan))
        if rc != _lib.OK:
            self._plan = None
            raise _lib.CrtfxError(rc, (self.lib.crtfx_egress_last_error(None) or b"").decode())
        assert self.lib.crtfx_egress_frame_bytes(self._plan) == self.frame_bytes

    def _check(self, rc):
        if rc != _lib.OK:
            raise _lib.CrtfxError(rc, (self.lib.crtfx_egress_last_error(self._plan) or b"").decode())

    def set_option(self, option: int, value: int) -> None:
        """Testing / A-B switches (crtfx_egress_option), e.g. set_option(_lib.EGRESS_OPT_FORCE_GENERAL, 1)."""
        self._check(self.lib.crtfx_egress_set_option(self._plan, int(option), int(value)))

    def run(self, frames, out=None):
        import torch
        h, w = self.size
        if frames.dtype != torch.uint8:
            raise _lib.CrtfxError(_lib.E_UNSUPPORTED, f"only uint8 RGB frames are converted, got {frames.dtype}")
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (h, w, 3) or frames.device != self.device:
            raise ValueError(f"frames must be uint8 [n, {h}, {w}, 3] on {self.device}, got {tuple(frames.shape)} on {frames.device}")
        n = int(frames.shape[0])
        if out is None:
            out = torch.empty((n, self.frame_bytes), dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or tuple(out.shape) != (n, self.frame_bytes) or out.device != self.device:
            raise ValueError(f"out must be uint8 [{n}, {self.frame_bytes}] on {self.device}")
        for name, t in (("frames", frames), ("out", out)):
            if n and not t[0].is_contiguous():
                raise ValueError(f"every frame of `{name}` must be contiguous (only the batch stride is free)")
        if n == 0:
            return out
        with torch.cuda.device(self.device):
            self._check(self.lib.crtfx_egress_run(self._plan, frames.data_ptr(), frames.stride(0), out.data_ptr(), out.stride(0), n,
                                                  torch.cuda.current_stream(self.device).cuda_stream))
        return out

    def planes(self, out):
        """Views of `out` ([n, frame_bytes] or [frame_bytes]; a tensor or a numpy array): (Y, U, V) or (Y, UV) — see split_planes."""
        return split_planes(out, self.size, self.layout)

    def plan(self) -> dict:
        """crtfx_egress_last_plan as a dictionary, e.g. {"egress": "k_egress_420<nv12,vec>", "frames": "5"}."""
        buf = ctypes.create_string_buffer(256)
        self._check(self.lib.crtfx_egress_last_plan(self._plan, buf, len(buf)))
        return dict(kv.split("=", 1) for kv in buf.value.decode().split(";") if kv)

    def close(self) -> None:
        if getattr(self, "_plan", None):
            self.lib.crtfx_egress_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 - interpreter shutdown
            pass
