"""`UnpackYuv422` and `EgressYuv422` — `UnpackYuv` and `EgressYuv` for the 8-bit 4:2:2 formats: what capture cards and HDMI / SDI grabbers
deliver (packed uyvy422 / yuyv422) and what mezzanine and broadcast codecs decode to (planar yuv422p), 2 bytes per pixel.  In front of the
chain such frames become the uint8 RGB frames it takes; behind it the finished frames become 4:2:2 again, several frames per launch
(include/crtfx_422.h holds the layouts, the arithmetic and the two kernel paths of each direction).  The host builds the integer matrices
(tables.rgb_matrix / tables.yuv_matrix, the 4:2:0 stages' own); the library copies them.  Not byte-equal to libswscale — see the header."""
from __future__ import annotations

import ctypes
from typing import Tuple

from . import _lib, tables

LAYOUTS = {"yuv422p": _lib.YUV422_YUV422P, "yuyv422": _lib.YUV422_YUYV422, "uyvy422": _lib.YUV422_UYVY422}
_MACROPIXEL = {"yuyv422": (0, 2, 1, 3), "uyvy422": (1, 3, 0, 2)}      # byte positions of Y0, Y1, U, V


def _layout(layout):
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, got {layout!r}")
    return layout


def frame_bytes(h: int, w: int, layout: str) -> int:
    """Bytes of one h x w frame, rows unpadded: h * w + 2 * h * ceil(w / 2) for yuv422p, 4 * h * ceil(w / 2) for yuyv422 / uyvy422 (an
    odd row ends in a macropixel whose second luma byte is padding)."""
    h, w, cw = int(h), int(w), (int(w) + 1) // 2
    return h * w + 2 * h * cw if _layout(layout) == "yuv422p" else 4 * h * cw


def split_planes(packed, size: Tuple[int, int], layout: str):
    """Views of `packed` ([..., frame_bytes]; a tensor or a numpy array) for an h x w frame: (Y [.., h, w], U [.., h, cw], V [.., h, cw])
    with cw = ceil(w / 2).  For yuyv422 / uyvy422 the three are strided views into the macropixels (Y of an odd row leaves the pad byte out)."""
    h, w = int(size[0]), int(size[1])
    cw = (w + 1) // 2
    fb = frame_bytes(h, w, layout)
    if int(packed.shape[-1]) != fb:
        raise ValueError(f"the last axis must hold {fb} bytes, got {tuple(packed.shape)}")
    lead = tuple(packed.shape[:-1])
    if layout == "yuv422p":
        return (packed[..., :h * w].reshape(lead + (h, w)), packed[..., h * w:h * w + h * cw].reshape(lead + (h, cw)),
                packed[..., h * w + h * cw:].reshape(lead + (h, cw)))
    y0, _, u, v = _MACROPIXEL[layout]
    mp = packed.reshape(lead + (h, cw, 4))
    rows = packed.reshape(lead + (h, 2 * cw, 2))                       # (luma, chroma) or (chroma, luma) byte pairs
    return rows[..., :w, y0], mp[..., u], mp[..., v]


class _Yuv422:
    """What the two plans share: the handle of one crtfx_<family>_* family."""
    _family = ""
    _force_option = 1

    def __init__(self, device, size, layout, matrix, range, pix_fmt, table, force_general):     # noqa: A002 - the issue's keyword
        import torch
        self.lib = _lib.load()
        self._fn = lambda name: getattr(self.lib, f"crtfx_{self._family}_{name}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"{type(self).__name__} needs a ROCm device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        _layout(layout)
        self.size = (int(size[0]), int(size[1]))
        self.layout, self.matrix, self.range = layout, matrix, range
        if min(self.size) < 1:
            raise _lib.CrtfxError(_lib.E_INVALID, f"size {self.size} must be at least 1 x 1")
        m, off = table(matrix, range)
        self.frame_bytes = frame_bytes(self.size[0], self.size[1], layout)
        self._plan = ctypes.c_void_p()
        rc = self._fn("create")(self.device.index, self.size[0], self.size[1], int(pix_fmt), LAYOUTS[layout], tables.ptr(m), tables.ptr(off),
                                ctypes.byref(self._plan))
        if rc != _lib.OK:
            self._plan = None
            raise _lib.CrtfxError(rc, (self._fn("last_error")(None) or b"").decode())
        assert self._fn("frame_bytes")(self._plan) == self.frame_bytes
        self._force_general = False
        if force_general:
            self.force_general = True

    def _check(self, rc):
        if rc != _lib.OK:
            raise _lib.CrtfxError(rc, (self._fn("last_error")(self._plan) or b"").decode())

    def set_option(self, option: int, value: int) -> None:
        """Testing / A-B switches, e.g. set_option(_lib.UNPACK422_OPT_FORCE_GENERAL, 1) / set_option(_lib.EGRESS422_OPT_FORCE_GENERAL, 1)."""
        self._check(self._fn("set_option")(self._plan, int(option), int(value)))
        if int(option) == self._force_option:
            self._force_general = bool(value)

    @property
    def force_general(self) -> bool:
        """Take the byte-access kernel whatever the width and alignment (*_OPT_FORCE_GENERAL)."""
        return self._force_general

    @force_general.setter
    def force_general(self, value) -> None:
        self.set_option(self._force_option, 1 if value else 0)

    def _run(self, src, dst, n):
        import torch
        for name, t in (("input", src), ("out", dst)):
            if n and not t[0].is_contiguous():
                raise ValueError(f"every frame of the {name} must be contiguous (only the batch stride is free)")
        if n == 0:
            return dst
        with torch.cuda.device(self.device):
            self._check(self._fn("run")(self._plan, src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), n,
                                        torch.cuda.current_stream(self.device).cuda_stream))
        return dst

    def __call__(self, src, out=None):
        return self.run(src, out)

    def planes(self, packed):
        """Views of `packed` ([n, frame_bytes] or [frame_bytes]; a tensor or a numpy array): (Y, U, V) — see split_planes."""
        return split_planes(packed, self.size, self.layout)

    def last_plan(self) -> str:
        """crtfx_<family>_last_plan, e.g. "unpack422=k_unpack_422<uyvy422,vec>;frames=5"."""
        buf = ctypes.create_string_buffer(256)
        self._check(self._fn("last_plan")(self._plan, buf, len(buf)))
        return buf.value.decode()

    def plan(self) -> dict:
        """last_plan() as a dictionary, e.g. {"unpack422": "k_unpack_422<uyvy422,vec>", "frames": "5"}."""
        return dict(kv.split("=", 1) for kv in self.last_plan().split(";") if kv)

    def close(self) -> None:
        if getattr(self, "_plan", None):
            self._fn("destroy")(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 - interpreter shutdown
            pass


class UnpackYuv422(_Yuv422):
    """plan = UnpackYuv422(device, (h, w), layout, matrix="bt601", rng="tv"); rgb = plan(packed_u8[n, frame_bytes]) -> uint8[n, h, w, 3]
    (plan.run is the same call).  `packed` and `out` are tensors on `device` whose frames are contiguous (the batch stride is free: slices of
    larger tensors are fine).  The work is enqueued on the current stream of `device`; nothing synchronises.
    `rng` ("tv" / "pc") is the name of the range argument; `range=` is accepted only so that a call written for UnpackYuv / EgressYuv
    (which spell it that way, as process_frames and the CLI do) works unchanged — when both are given, `range` is the one used."""
    _family = "unpack422"
    _force_option = _lib.UNPACK422_OPT_FORCE_GENERAL

    def __init__(self, device, size: Tuple[int, int], layout: str, matrix: str = "bt601", rng: str = "tv", pix_fmt: int = _lib.PIX_U8,
                 force_general: bool = False, range: str = None):        # noqa: A002 - `range`: the 4:2:0 classes' name for `rng`
        super().__init__(device, size, layout, matrix, rng if range is None else range, pix_fmt, tables.rgb_matrix, force_general)

    def run(self, packed, out=None):
        import torch
        h, w = self.size
        if packed.dtype != torch.uint8:
            raise _lib.CrtfxError(_lib.E_UNSUPPORTED, f"only uint8 {self.layout} frames are converted, got {packed.dtype}")
        if packed.dim() != 2 or int(packed.shape[1]) != self.frame_bytes or packed.device != self.device:
            raise ValueError(f"packed must be uint8 [n, {self.frame_bytes}] on {self.device}, got {tuple(packed.shape)} on {packed.device}")
        n = int(packed.shape[0])
        if out is None:
            out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w, 3) or out.device != self.device:
            raise ValueError(f"out must be uint8 [{n}, {h}, {w}, 3] on {self.device}")
        return self._run(packed, out, n)


class EgressYuv422(_Yuv422):
    """plan = EgressYuv422(device, (h, w), layout, matrix="bt601", rng="tv"); out = plan(frames_u8[n, h, w, 3]) -> uint8[n, frame_bytes].
    The rules of UnpackYuv422, the `rng` / `range` spelling included."""
    _family = "egress422"
    _force_option = _lib.EGRESS422_OPT_FORCE_GENERAL

    def __init__(self, device, size: Tuple[int, int], layout: str, matrix: str = "bt601", rng: str = "tv", pix_fmt: int = _lib.PIX_U8,
                 force_general: bool = False, range: str = None):        # noqa: A002 - `range`: the 4:2:0 classes' name for `rng`
        super().__init__(device, size, layout, matrix, rng if range is None else range, pix_fmt, tables.yuv_matrix, force_general)

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
        return self._run(frames, out, n)
