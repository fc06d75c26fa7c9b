"""`UnpackYuv422` and `EgressYuv422` — `UnpackYuv` and `EgressYuv` for the 8-bit 4:2:2 formats: what capture cards and HDMI / SDI grabbers
deliver (packed uyvy422 / yuyv422) and what mezzanine and broadcast codecs decode to (planar yuv422p), 2 bytes per pixel.  In front of the
chain such frames become the uint8 RGB frames it takes; behind it the finished frames become 4:2:2 again, several frames per launch
(include/crtfx_422.h holds the layouts, the arithmetic and the two kernel paths of each direction).  The host builds the integer matrices
(tables.rgb_matrix / tables.yuv_matrix, the 4:2:0 stages' own); the library copies them.  Not byte-equal to libswscale — see the header."""
from __future__ import annotations

from typing import Tuple

from . import _lib, tables
from ._stage import EgressPlan, SourcePlan

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
    """What the two plans share.  `rng` ("tv" / "pc") is the name of the range argument; `range=` is accepted only so that a call written
    for UnpackYuv / EgressYuv (which spell it that way, as process_frames and the CLI do) works unchanged — when both are given, `range`
    is the one used."""
    _layouts, _split_planes, _frame_bytes = LAYOUTS, split_planes, frame_bytes

    def __init__(self, device, size: Tuple[int, int], layout: str, matrix: str = "bt601", rng: str = "tv", pix_fmt: int = _lib.PIX_U8,
                 force_general: bool = False, range: str = None):        # noqa: A002 - `range`: the 4:2:0 classes' name for `rng`
        super().__init__(device, size, layout, matrix, rng if range is None else range, pix_fmt, force_general)


class UnpackYuv422(_Yuv422, SourcePlan):
    """plan = UnpackYuv422(device, (h, w), layout, matrix="bt601", rng="tv"); rgb = plan(packed_u8[n, frame_bytes]) -> uint8[n, h, w, 3]
    (plan.run is the same call).  `packed` and `out` are tensors on `device` whose frames are contiguous (the batch stride is free: slices of
    larger tensors are fine).  The work is enqueued on the current stream of `device`; nothing synchronises."""
    _family, _force_option, _table = "unpack422", _lib.UNPACK422_OPT_FORCE_GENERAL, tables.rgb_matrix


class EgressYuv422(_Yuv422, EgressPlan):
    """plan = EgressYuv422(device, (h, w), layout, matrix="bt601", rng="tv"); out = plan(frames_u8[n, h, w, 3]) -> uint8[n, frame_bytes].
    The rules of UnpackYuv422, the `rng` / `range` spelling included."""
    _family, _force_option, _table = "egress422", _lib.EGRESS422_OPT_FORCE_GENERAL, tables.yuv_matrix
