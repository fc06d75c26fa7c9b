"""`UnpackDeep444` and `EgressDeep444` — `UnpackYuv10` and `EgressYuv10` for full-resolution deep colour: yuv444p10le (ProRes 4444 /
DNxHR 444 decodes), gbrp10le (DPX / TIFF / EXR sequences through ffmpeg) and x2rgb10le (10-bit screen and KMS capture).  In front of a
chain that runs on half pixels (FramePipeline(dtype=torch.float16)) such frames become half RGB frames on the 0..255 scale, behind it the
finished half frames become 10-bit 4:4:4 again, several frames per launch (include/crtfx_444.h holds the two memory layouts, the
arithmetic and the two kernel paths of each direction).  The three formats differ only in layout and table: yuv444p10le takes
tables.rgb_matrix10 / tables.yuv_matrix10 with the `matrix` and `range` keywords; for gbrp10le and x2rgb10le, which are full-range RGB
(tables.rgb_scale10), those two keywords do not apply and are ignored.  Packed frames travel as uint8 tensors of frame_bytes bytes: the
16-bit and 32-bit words are little-endian.  Not byte-equal to libswscale — see the header."""
from __future__ import annotations

import ctypes
from typing import Tuple

from . import _lib, tables

FORMATS = {"yuv444p10le": _lib.DEEP444_PLANAR, "gbrp10le": _lib.DEEP444_PLANAR, "x2rgb10le": _lib.DEEP444_X2RGB10LE}    # format -> C layout
_RGB_ORDER = {"gbrp10le": "gbr", "x2rgb10le": "rgb"}


def _fmt(fmt):
    if fmt not in FORMATS:
        raise ValueError(f"the format must be one of {sorted(FORMATS)}, got {fmt!r}")
    return fmt


def frame_bytes(h: int, w: int, fmt: str) -> int:
    """Bytes of one h x w frame, rows unpadded: 6 * h * w for yuv444p10le / gbrp10le (three planes of 16-bit words), 4 * h * w for
    x2rgb10le (one 32-bit word per pixel)."""
    return int(h) * int(w) * (4 if _fmt(fmt) == "x2rgb10le" else 6)


def split_planes(packed, size: Tuple[int, int], fmt: str):
    """Views of `packed` ([..., frame_bytes] uint8; a tensor or a numpy array, the last axis contiguous and aligned to its words) for an
    h x w frame, the words as stored.  yuv444p10le: (Y, U, V), gbrp10le: (G, B, R), each [.., h, w] 16-bit words (numpy: uint16, torch:
    int16 — the same bits; a sample is word & 1023).  x2rgb10le: (W,), [.., h, w] 32-bit words (numpy: uint32, torch: int32) with
    R = (W >> 20) & 1023, G = (W >> 10) & 1023, B = W & 1023."""
    import numpy as np
    h, w = int(size[0]), int(size[1])
    fb = frame_bytes(h, w, fmt)
    if int(packed.shape[-1]) != fb:
        raise ValueError(f"the last axis must hold {fb} bytes, got {tuple(packed.shape)}")
    lead = tuple(packed.shape[:-1])
    wide = fmt == "x2rgb10le"
    if isinstance(packed, np.ndarray):
        words = packed.view(np.uint32 if wide else np.uint16)
    else:
        import torch
        words = packed.view(torch.int32 if wide else torch.int16)
    if wide:
        return (words.reshape(lead + (h, w)),)
    return tuple(words[..., j * h * w:(j + 1) * h * w].reshape(lead + (h, w)) for j in range(3))


class _Deep444:
    """What the two plans share: the handle of one crtfx_<family>_* family."""
    _family = ""
    _egress = 0

    def __init__(self, device, size, layout, matrix, range, pix_fmt):     # noqa: A002 - the keyword of the other stages
        import torch
        self.lib = _lib.load()
        self._fn = lambda name: getattr(self.lib, f"crtfx_{self._family}_{name}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"{type(self).__name__} needs a ROCm device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        _fmt(layout)
        self.size = (int(size[0]), int(size[1]))
        self.layout, self.matrix, self.range = layout, matrix, range
        if min(self.size) < 1:
            raise _lib.CrtfxError(_lib.E_INVALID, f"size {self.size} must be at least 1 x 1")
        if layout in _RGB_ORDER:                 # full-range RGB: `matrix` and `range` do not apply
            m, off = tables.rgb_scale10(_RGB_ORDER[layout])[self._egress]
        else:
            m, off = (tables.yuv_matrix10 if self._egress else tables.rgb_matrix10)(matrix, range)
        self.frame_bytes = frame_bytes(self.size[0], self.size[1], layout)
        self._plan = ctypes.c_void_p()
        rc = self._fn("create")(self.device.index, self.size[0], self.size[1], int(pix_fmt), FORMATS[layout], tables.ptr(m), tables.ptr(off),
                                ctypes.byref(self._plan))
        if rc != _lib.OK:
            self._plan = None
            raise _lib.CrtfxError(rc, (self._fn("last_error")(None) or b"").decode())
        assert self._fn("frame_bytes")(self._plan) == self.frame_bytes

    def _check(self, rc):
        if rc != _lib.OK:
            raise _lib.CrtfxError(rc, (self._fn("last_error")(self._plan) or b"").decode())

    def set_option(self, option: int, value: int) -> None:
        """Testing / A-B switches, e.g. set_option(_lib.UNPACK444_OPT_FORCE_GENERAL, 1) / set_option(_lib.EGRESS444_OPT_FORCE_GENERAL, 1)."""
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
        """Word views of `packed` ([n, frame_bytes] or [frame_bytes] uint8; a tensor or a numpy array) — see split_planes."""
        return split_planes(packed, self.size, self.layout)

    def plan(self) -> dict:
        """crtfx_<family>_last_plan as a dictionary, e.g. {"unpack444": "k_unpack10_444<planar,vec>", "frames": "5"}."""
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


class UnpackDeep444(_Deep444):
    """plan = UnpackDeep444(device, (h, w), layout="yuv444p10le", matrix="bt601", range="tv"); rgb = plan.run(packed_u8[n, frame_bytes]) ->
    float16[n, h, w, 3] on the 0..255 scale.  `layout` is the format name: "yuv444p10le", "gbrp10le" or "x2rgb10le"; `matrix` and `range`
    apply to yuv444p10le only.  `packed` and `out` are tensors on `device` whose frames are contiguous (the batch stride is free: slices
    of larger tensors are fine; bases and strides must be even, and multiples of 4 on the x2rgb10le side).  The work is enqueued on the
    current stream of `device`; nothing synchronises."""
    _family = "unpack444"
    _egress = 0

    def __init__(self, device, size: Tuple[int, int], layout: str = "yuv444p10le", matrix: str = "bt601", range: str = "tv",    # noqa: A002
                 pix_fmt: int = _lib.PIX_F16):
        super().__init__(device, size, layout, matrix, range, pix_fmt)

    def run(self, packed, out=None):
        import torch
        h, w = self.size
        if packed.dtype != torch.uint8:
            raise _lib.CrtfxError(_lib.E_UNSUPPORTED, f"packed {self.layout} frames are uint8 tensors of frame_bytes bytes, got {packed.dtype}")
        if packed.dim() != 2 or int(packed.shape[1]) != self.frame_bytes or packed.device != self.device:
            raise ValueError(f"packed must be uint8 [n, {self.frame_bytes}] on {self.device}, got {tuple(packed.shape)} on {packed.device}")
        n = int(packed.shape[0])
        if out is None:
            out = torch.empty((n, h, w, 3), dtype=torch.float16, device=self.device)
        if out.dtype != torch.float16 or tuple(out.shape) != (n, h, w, 3) or out.device != self.device:
            raise ValueError(f"out must be float16 [{n}, {h}, {w}, 3] on {self.device}")
        return self._run(packed, out, n)


class EgressDeep444(_Deep444):
    """plan = EgressDeep444(device, (h, w), layout="yuv444p10le", matrix="bt601", range="tv"); out = plan.run(frames_f16[n, h, w, 3]) ->
    uint8[n, frame_bytes].  The rules of UnpackDeep444."""
    _family = "egress444"
    _egress = 1

    def __init__(self, device, size: Tuple[int, int], layout: str = "yuv444p10le", matrix: str = "bt601", range: str = "tv",    # noqa: A002
                 pix_fmt: int = _lib.PIX_F16):
        super().__init__(device, size, layout, matrix, range, pix_fmt)

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
