"""`UnpackYuv10` and `EgressYuv10` — `UnpackYuv` and `EgressYuv` for a chain that runs on half pixels (FramePipeline(dtype=torch.float16)):
10-bit 4:2:0 frames as decoders hand them out and encoders take them — planar yuv420p10le (software) or semi-planar p010le (hardware), 3
bytes per pixel — become half RGB frames on the 0..255 scale in front of the chain, and its finished half frames become 10-bit 4:2:0 behind
it, several frames per launch (include/crtfx_deep.h holds the arithmetic and the two kernel paths of each direction).  The host builds the
integer matrices (tables.rgb_matrix10 / tables.yuv_matrix10); the library copies them.  Packed frames travel as uint8 tensors of
frame_bytes bytes, as the 8-bit stages' do: the 16-bit words are little-endian.  Not byte-equal to libswscale — see the header."""
from __future__ import annotations

import ctypes
from typing import Tuple

from . import _lib, tables

LAYOUTS = {"yuv420p10le": _lib.DEEP_YUV420P10LE, "p010le": _lib.DEEP_P010LE}


def frame_bytes(h: int, w: int) -> int:
    """Bytes of one h x w yuv420p10le / p010le frame: 2 * (h * w + 2 * ceil(h / 2) * ceil(w / 2))."""
    return 2 * (int(h) * int(w) + 2 * ((int(h) + 1) // 2) * ((int(w) + 1) // 2))


def _words(packed):
    """`packed` ([..., frame_bytes] uint8, or already 16-bit words; a tensor or a numpy array) as 16-bit words: uint16 (numpy) or int16 (torch)."""
    import numpy as np
    if isinstance(packed, np.ndarray):
        return packed.view(np.uint16) if packed.dtype == np.uint8 else packed
    import torch
    return packed.view(torch.int16) if packed.dtype == torch.uint8 else packed


def split_planes(packed, size: Tuple[int, int], layout: str):
    """Views of `packed` ([..., frame_bytes] uint8; a tensor or a numpy array, the last axis contiguous and 2-byte aligned) for an h x w
    frame, as 16-bit words (numpy: uint16, torch: int16 — the same bits): (Y [.., h, w], U [.., ch, cw], V [.., ch, cw]) for yuv420p10le,
    (Y, UV [.., ch, cw, 2]) for p010le, with ch = ceil(h / 2) and cw = ceil(w / 2).  The words are as stored: a p010le sample is word >> 6."""
    h, w = int(size[0]), int(size[1])
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, got {layout!r}")
    if int(packed.shape[-1]) != frame_bytes(h, w):
        raise ValueError(f"the last axis must hold {frame_bytes(h, w)} bytes, got {tuple(packed.shape)}")
    out = _words(packed)
    lead = tuple(out.shape[:-1])
    y = out[..., :h * w].reshape(lead + (h, w))
    if layout == "p010le":
        return y, out[..., h * w:].reshape(lead + (ch, cw, 2))
    return y, out[..., h * w:h * w + ch * cw].reshape(lead + (ch, cw)), out[..., h * w + ch * cw:].reshape(lead + (ch, cw))


class _Deep:
    """What the two plans share: the handle of one crtfx_<family>_* family."""
    _family = ""

    def __init__(self, device, size, layout, matrix, range, pix_fmt, table):     # noqa: A002 - the issue's keyword
        import torch
        self.lib = _lib.load()
        self._fn = lambda name: getattr(self.lib, f"crtfx_{self._family}_{name}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"{type(self).__name__} needs a ROCm device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if layout not in LAYOUTS:
            raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, got {layout!r}")
        self.size = (int(size[0]), int(size[1]))
        self.layout, self.matrix, self.range = layout, matrix, range
        if min(self.size) < 1:
            raise _lib.CrtfxError(_lib.E_INVALID, f"size {self.size} must be at least 1 x 1")
        m, off = table(matrix, range)
        self.frame_bytes = frame_bytes(*self.size)
        self._plan = ctypes.c_void_p()
        rc = self._fn("create")(self.device.index, self.size[0], self.size[1], int(pix_fmt), LAYOUTS[layout], tables.ptr(m), tables.ptr(off),
                                ctypes.byref(self._plan))
        if rc != _lib.OK:
            self._plan = None
            raise _lib.CrtfxError(rc, (self._fn("last_error")(None) or b"").decode())
        assert self._fn("frame_bytes")(self._plan) == self.frame_bytes

    def _check(self, rc):
        if rc != _lib.OK:
            raise _lib.CrtfxError(rc, (self._fn("last_error")(self._plan) or b"").decode())

    def set_option(self, option: int, value: int) -> None:
        """Testing / A-B switches, e.g. set_option(_lib.UNPACK10_OPT_FORCE_GENERAL, 1) / set_option(_lib.EGRESS10_OPT_FORCE_GENERAL, 1)."""
        self._check(self._fn("set_option")(self._plan, int(option), int(value)))

    def _run(self, src, dst, n):
        import torch
        for name, t in (("input", src), ("out", dst)):
            if n and not t[0].is_contiguous():
                raise ValueError(f"every frame of the {name} must be contiguous (only the batch stride is free)")
        if n == 0:
            return dst
        with torch.cuda.device(self.device):
            self._check(self._fn("run")(self._plan, src.data_ptr(), src.stride(0) * src.element_size(), dst.data_ptr(),
                                        dst.stride(0) * dst.element_size(), n, torch.cuda.current_stream(self.device).cuda_stream))
        return dst

    def planes(self, packed):
        """16-bit views of `packed` ([n, frame_bytes] or [frame_bytes] uint8; a tensor or a numpy array): (Y, U, V) or (Y, UV) — see split_planes."""
        return split_planes(packed, self.size, self.layout)

    def plan(self) -> dict:
        """crtfx_<family>_last_plan as a dictionary, e.g. {"unpack10": "k_unpack10_420<p010le,vec>", "frames": "5"}."""
        buf = ctypes.create_string_buffer(256)
        self._check(self._fn("last_plan")(self._plan, buf, len(buf)))
        return dict(kv.split("=", 1) for kv in buf.value.decode().split(";") if kv)

    def close(self) -> None:
        if getattr(self, "_plan", None):
            self._fn("destroy")(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 - interpreter shutdown
            pass


class UnpackYuv10(_Deep):
    """plan = UnpackYuv10(device, (h, w), layout="yuv420p10le", matrix="bt601", range="tv"); rgb = plan.run(packed_u8[n, frame_bytes]) ->
    float16[n, h, w, 3] on the 0..255 scale.  `packed` and `out` are tensors on `device` whose frames are contiguous (the batch stride is
    free: slices of larger tensors are fine; bases and strides must be even).  The work is enqueued on the current stream of `device`;
    nothing synchronises."""
    _family = "unpack10"

    def __init__(self, device, size: Tuple[int, int], layout: str = "yuv420p10le", matrix: str = "bt601", range: str = "tv",    # noqa: A002
                 pix_fmt: int = _lib.PIX_F16):
        super().__init__(device, size, layout, matrix, range, pix_fmt, tables.rgb_matrix10)

    def run(self, packed, out=None):
        import torch
        h, w = self.size
        if packed.dtype != torch.uint8:
            raise _lib.CrtfxError(_lib.E_UNSUPPORTED, f"packed yuv420p10le / p010le frames are uint8 tensors of frame_bytes bytes, got {packed.dtype}")
        if packed.dim() != 2 or int(packed.shape[1]) != self.frame_bytes or packed.device != self.device:
            raise ValueError(f"packed must be uint8 [n, {self.frame_bytes}] on {self.device}, got {tuple(packed.shape)} on {packed.device}")
        n = int(packed.shape[0])
        if out is None:
            out = torch.empty((n, h, w, 3), dtype=torch.float16, device=self.device)
        if out.dtype != torch.float16 or tuple(out.shape) != (n, h, w, 3) or out.device != self.device:
            raise ValueError(f"out must be float16 [{n}, {h}, {w}, 3] on {self.device}")
        return self._run(packed, out, n)


class EgressYuv10(_Deep):
    """plan = EgressYuv10(device, (h, w), layout="yuv420p10le", matrix="bt601", range="tv"); out = plan.run(frames_f16[n, h, w, 3]) ->
    uint8[n, frame_bytes].  The rules of UnpackYuv10."""
    _family = "egress10"

    def __init__(self, device, size: Tuple[int, int], layout: str = "yuv420p10le", matrix: str = "bt601", range: str = "tv",    # noqa: A002
                 pix_fmt: int = _lib.PIX_F16):
        super().__init__(device, size, layout, matrix, range, pix_fmt, tables.yuv_matrix10)

    def run(self, frames, out=None):
        import torch
        h, w = self.size
        if frames.dtype != torch.float16:
            raise _lib.CrtfxError(_lib.E_UNSUPPORTED, f"only half RGB frames are converted, got {frames.dtype}")
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (h, w, 3) or frames.device != self.device:
            raise ValueError(f"frames must be float16 [n, {h}, {w}, 3] on {self.device}, got {tuple(frames.shape)} on {frames.device}")
        n = int(frames.shape[0])
        if out is None:
            out = torch.empty((n, self.frame_bytes), dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or tuple(out.shape) != (n, self.frame_bytes) or out.device != self.device:
            raise ValueError(f"out must be uint8 [{n}, {self.frame_bytes}] on {self.device}")
        return self._run(frames, out, n)
