"""`EgressYuv` — the last step of the reference's render loop on the device: each of its encoder branches ends in `-pix_fmt yuv420p`
(crt_filter.py ref:970-1002), so every finished rgb24 frame is converted to 4:2:0 by libswscale on one host core.  Here finished uint8 RGB
frames in HBM become yuv420p (I420) or nv12 frames of 1.5 bytes per pixel, several frames per launch (include/crtfx_egress.h holds the
arithmetic and the two kernel paths).  The host builds the integer matrix (tables.yuv_matrix); the library copies it.  Not byte-equal to
libswscale — see the header."""
from __future__ import annotations

from typing import Tuple

from . import _lib, tables
from ._stage import EgressPlan

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


class EgressYuv(EgressPlan):
    """plan = EgressYuv(device, (h, w), layout="yuv420p", matrix="bt601", range="tv"); out = plan.run(frames_u8[n, h, w, 3]) ->
    uint8[n, frame_bytes].  `frames` and `out` are tensors on `device` whose frames are contiguous (the batch stride is free: slices of
    larger tensors are fine).  The work is enqueued on the current stream of `device`; nothing synchronises."""
    _family, _force_option, _layouts = "egress", _lib.EGRESS_OPT_FORCE_GENERAL, LAYOUTS
    _table, _split_planes = tables.yuv_matrix, split_planes
    _frame_bytes = lambda h, w, layout: frame_bytes(h, w)     # noqa: E731

    def __init__(self, device, size: Tuple[int, int], layout: str = "yuv420p", matrix: str = "bt601", range: str = "tv",    # noqa: A002 - the issue's keyword
                 pix_fmt: int = _lib.PIX_U8):
        super().__init__(device, size, layout, matrix, range, pix_fmt)
