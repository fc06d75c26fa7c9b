"""`UnpackYuv` — the step in front of the reference's render loop on the device: no decoder produces rgb24 (software decoders hand out
yuv420p, hardware decoders nv12), so every user of the reference's `FFmpegRawReader` (ref:469-514) puts `-pix_fmt rgb24` in front of it and
libswscale converts every source frame on one host core.  Here uint8 yuv420p (I420) or nv12 frames in HBM, 1.5 bytes per pixel, become the
uint8 RGB frames the chain takes, several frames per launch (include/crtfx_unpack.h holds the arithmetic and the two kernel paths).  The
host builds the integer matrix (tables.rgb_matrix); the library copies it.  The mirror image of `EgressYuv`; not byte-equal to libswscale
— see the header."""
from __future__ import annotations

from typing import Tuple

from . import _lib, tables
from ._stage import SourcePlan
from .egress import frame_bytes, split_planes  # noqa: F401 - the layout is the egress stage's, read instead of written

LAYOUTS = {"yuv420p": _lib.UNPACK_YUV420P, "nv12": _lib.UNPACK_NV12}


class UnpackYuv(SourcePlan):
    """plan = UnpackYuv(device, (h, w), layout="yuv420p", matrix="bt601", range="tv"); rgb = plan.run(packed_u8[n, frame_bytes]) ->
    uint8[n, h, w, 3].  `packed` and `out` are tensors on `device` whose frames are contiguous (the batch stride is free: slices of larger
    tensors are fine).  The work is enqueued on the current stream of `device`; nothing synchronises."""
    _family, _force_option, _layouts = "unpack", _lib.UNPACK_OPT_FORCE_GENERAL, LAYOUTS
    _table, _split_planes = tables.rgb_matrix, split_planes
    _frame_bytes = lambda h, w, layout: frame_bytes(h, w)     # noqa: E731

    def __init__(self, device, size: Tuple[int, int], layout: str = "yuv420p", matrix: str = "bt601", range: str = "tv",    # noqa: A002 - the issue's keyword
                 pix_fmt: int = _lib.PIX_U8):
        super().__init__(device, size, layout, matrix, range, pix_fmt)
