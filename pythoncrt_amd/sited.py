"""`UnpackSited` — the source stage of the seven sub-sampled formats (yuv420p / nv12, yuv422p / yuyv422 / uyvy422, yuv420p10le / p010le)
with the chroma planes interpolated at a stated siting instead of replicated over their pixels: "left" for what MPEG-2 / H.264 / HEVC
decoders hand out (ffprobe's chroma_location=left, or nothing), "center" for JPEG-family sources.  It stands where UnpackYuv, UnpackYuv422
and UnpackYuv10 stand — the same packed frames in, the same RGB frames out (uint8, or half for the two 10-bit layouts) — and gives their
bytes wherever the chroma taps of a pixel are equal (include/crtfx_sited.h holds the arithmetic and the two kernel paths).  The matrices
are those stages' (tables.rgb_matrix / tables.rgb_matrix10).  Not byte-equal to libswscale — see the header.

`EgressSited` — its mirror image behind the chain: finished RGB frames to the same seven formats with every chroma sample filtered onto the
stated siting ([1 2 1] / 4 around luma column 2 cx for "left") instead of taken as the box mean, which is centre siting.  It stands where
EgressYuv, EgressYuv422 and EgressYuv10 stand and gives their bytes, for every input, with siting="center"
(include/crtfx_egress_sited.h).  The matrices are those stages' (tables.yuv_matrix / tables.yuv_matrix10)."""
from __future__ import annotations

from typing import Tuple

from . import _lib, deep, egress, tables, yuv422
from ._stage import EgressPlan, SourcePlan

LAYOUTS = {"yuv420p": _lib.SITED_YUV420P, "nv12": _lib.SITED_NV12, "yuv422p": _lib.SITED_YUV422P, "yuyv422": _lib.SITED_YUYV422,
           "uyvy422": _lib.SITED_UYVY422, "yuv420p10le": _lib.SITED_YUV420P10LE, "p010le": _lib.SITED_P010LE}
SITINGS = {"left": _lib.SITED_LEFT, "center": _lib.SITED_CENTER}


def _module(layout):
    """The family module whose geometry the layout has."""
    return deep if layout in deep.LAYOUTS else yuv422 if layout in yuv422.LAYOUTS else egress


def frame_bytes(h: int, w: int, layout: str) -> int:
    """Bytes of one h x w frame of `layout`: the existing families' expressions."""
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, got {layout!r}")
    return yuv422.frame_bytes(h, w, layout) if layout in yuv422.LAYOUTS else _module(layout).frame_bytes(h, w)


def split_planes(packed, size: Tuple[int, int], layout: str):
    """Views of `packed` ([..., frame_bytes]) for an h x w frame: the family module's split_planes (egress / yuv422 / deep)."""
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, got {layout!r}")
    return _module(layout).split_planes(packed, size, layout)


class UnpackSited(SourcePlan):
    """plan = UnpackSited(device, (h, w), layout, matrix="bt601", range="tv", siting="left"); rgb = plan.run(packed_u8[n, frame_bytes]) ->
    uint8[n, h, w, 3], or float16[n, h, w, 3] on the 0..255 scale for "yuv420p10le" / "p010le".  `packed` and `out` are tensors on `device`
    whose frames are contiguous (the batch stride is free; 10-bit: bases and strides must be even).  `plan.siting = "center"` switches a
    live plan.  The work is enqueued on the current stream of `device`; nothing synchronises."""
    _family, _force_option, _layouts = "sited", _lib.SITED_OPT_FORCE_GENERAL, LAYOUTS
    _frame_bytes, _split_planes = frame_bytes, split_planes

    def __init__(self, device, size: Tuple[int, int], layout: str, matrix: str = "bt601", range: str = "tv", siting: str = "left",    # noqa: A002
                 force_general: bool = False):
        if siting not in SITINGS:
            raise ValueError(f"siting must be one of {sorted(SITINGS)}, got {siting!r}")
        ten = layout in deep.LAYOUTS
        self._rgb = "float16" if ten else "uint8"
        self._siting = "left"
        super().__init__(device, size, layout, matrix, range, _lib.PIX_F16 if ten else _lib.PIX_U8, force_general)
        if siting != "left":
            self.siting = siting

    def _tables(self):
        return (tables.rgb_matrix10 if self.layout in deep.LAYOUTS else tables.rgb_matrix)(self.matrix, self.range)

    def set_option(self, option: int, value: int) -> None:
        super().set_option(option, value)
        if int(option) == _lib.SITED_OPT_SITING:
            self._siting = "center" if int(value) == _lib.SITED_CENTER else "left"

    @property
    def siting(self) -> str:
        """"left" or "center": where a chroma sample sits against its two luma columns (CRTFX_SITED_OPT_SITING)."""
        return self._siting

    @siting.setter
    def siting(self, value: str) -> None:
        if value not in SITINGS:
            raise ValueError(f"siting must be one of {sorted(SITINGS)}, got {value!r}")
        self.set_option(_lib.SITED_OPT_SITING, SITINGS[value])


class EgressSited(EgressPlan):
    """plan = EgressSited(device, (h, w), layout, matrix="bt601", range="tv", siting="left"); out = plan.run(frames[n, h, w, 3]) ->
    uint8[n, frame_bytes]; `frames` are uint8, or float16 on the 0..255 scale for "yuv420p10le" / "p010le".  `frames` and `out` are tensors
    on `device` whose frames are contiguous (the batch stride is free; 10-bit: bases and strides must be even).  `plan.siting = "center"`
    switches a live plan to the box stages' bytes.  The work is enqueued on the current stream of `device`; nothing synchronises."""
    _family, _force_option, _layouts = "egress_sited", _lib.EGRESS_SITED_OPT_FORCE_GENERAL, LAYOUTS
    _frame_bytes, _split_planes = frame_bytes, split_planes

    def __init__(self, device, size: Tuple[int, int], layout: str, matrix: str = "bt601", range: str = "tv", siting: str = "left",    # noqa: A002
                 force_general: bool = False):
        if siting not in SITINGS:
            raise ValueError(f"siting must be one of {sorted(SITINGS)}, got {siting!r}")
        ten = layout in deep.LAYOUTS
        self._rgb = "float16" if ten else "uint8"
        self._siting = "left"
        super().__init__(device, size, layout, matrix, range, _lib.PIX_F16 if ten else _lib.PIX_U8, force_general)
        if siting != "left":
            self.siting = siting

    def _tables(self):
        return (tables.yuv_matrix10 if self.layout in deep.LAYOUTS else tables.yuv_matrix)(self.matrix, self.range)

    def set_option(self, option: int, value: int) -> None:
        super().set_option(option, value)
        if int(option) == _lib.EGRESS_SITED_OPT_SITING:
            self._siting = "center" if int(value) == _lib.SITED_CENTER else "left"

    @property
    def siting(self) -> str:
        """"left" or "center": where a chroma sample sits against its two luma columns (CRTFX_EGRESS_SITED_OPT_SITING)."""
        return self._siting

    @siting.setter
    def siting(self, value: str) -> None:
        if value not in SITINGS:
            raise ValueError(f"siting must be one of {sorted(SITINGS)}, got {value!r}")
        self.set_option(_lib.EGRESS_SITED_OPT_SITING, SITINGS[value])
