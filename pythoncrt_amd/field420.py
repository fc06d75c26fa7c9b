"""`UnpackField420` — the source stage of INTERLACED 4:2:0 material (yuv420p / nv12 / yuv420p10le / p010le): every luma row takes its chroma
from rows of its own field only — chroma rows 0, 2, 4, ... are the top field's, rows 1, 3, 5, ... the bottom field's, as an interlaced
encoder sub-samples them — where UnpackYuv, UnpackYuv10 and UnpackSited pair the two fields under every chroma row.  It stands where they
stand — the same packed frames in, the same RGB frames out (uint8, or half for the two 10-bit layouts) — in front of a deinterlacer, which
then reads fields whose colour is their own.  `chroma` is "replicate" (the nearest chroma row of the field, the pixel's own column), or
"left" / "center": interpolated at MPEG-2's interlaced vertical siting and that horizontal siting (include/crtfx_field420.h holds the
arithmetic and the two kernel paths).  The matrices are the other source stages' (tables.rgb_matrix / tables.rgb_matrix10).  Not byte-equal
to libswscale — see the header.

`EgressField420` — its mirror image behind the chain, for INTERLACED 4:2:0 deliveries: finished (woven) RGB frames to the same four layouts
with every chroma sample formed from luma rows of its own field — chroma rows 0, 2, 4, ... from the top field's rows, rows 1, 3, 5, ... from
the bottom field's, as an interlaced decoder reads them — where EgressYuv, EgressYuv10 and EgressSited mix one row of each field into
every sample.  It stands where they stand and, with chroma="center", gives the weave of their bytes for each field run as a frame of its
own; "left" is MPEG-2's interlaced siting (include/crtfx_egress_field420.h).  The matrices are those stages' (tables.yuv_matrix /
tables.yuv_matrix10).  The height is a multiple of 4."""
from __future__ import annotations

from typing import Tuple

from . import _lib, deep, egress, tables
from ._stage import EgressPlan, SourcePlan

LAYOUTS = {"yuv420p": _lib.FIELD420_YUV420P, "nv12": _lib.FIELD420_NV12, "yuv420p10le": _lib.FIELD420_YUV420P10LE, "p010le": _lib.FIELD420_P010LE}
CHROMAS = {"replicate": _lib.FIELD420_REPLICATE, "left": _lib.FIELD420_LEFT, "center": _lib.FIELD420_CENTER}
EGRESS_CHROMAS = {"center": _lib.EGRESS_FIELD420_CENTER, "left": _lib.EGRESS_FIELD420_LEFT}
MIN_ROWS = 4            # each field needs a chroma row of its own
EGRESS_ROWS = 4         # ... and on the way out whole pairs of its luma rows under every one: heights are multiples of this


def _module(layout):
    """The family module whose geometry the layout has."""
    return deep if layout in deep.LAYOUTS else egress


def frame_bytes(h: int, w: int, layout: str) -> int:
    """Bytes of one h x w frame of `layout`: the existing families' expressions."""
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, got {layout!r}")
    return _module(layout).frame_bytes(h, w)


def split_planes(packed, size: Tuple[int, int], layout: str):
    """Views of `packed` ([..., frame_bytes]) for an h x w frame: the family module's split_planes (egress / deep)."""
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, got {layout!r}")
    return _module(layout).split_planes(packed, size, layout)


class UnpackField420(SourcePlan):
    """plan = UnpackField420(device, (h, w), layout, matrix="bt601", range="tv", chroma="replicate"); rgb = plan.run(packed_u8[n, frame_bytes])
    -> uint8[n, h, w, 3], or float16[n, h, w, 3] on the 0..255 scale for "yuv420p10le" / "p010le".  h is even and at least 4.  `packed` and
    `out` are tensors on `device` whose frames are contiguous (the batch stride is free; 10-bit: bases and strides must be even).
    `plan.chroma = "left"` switches a live plan.  The work is enqueued on the current stream of `device`; nothing synchronises."""
    _family, _force_option, _layouts = "field420", _lib.FIELD420_OPT_FORCE_GENERAL, LAYOUTS
    _frame_bytes, _split_planes = frame_bytes, split_planes

    def __init__(self, device, size: Tuple[int, int], layout: str, matrix: str = "bt601", range: str = "tv", chroma: str = "replicate",    # noqa: A002
                 force_general: bool = False):
        if chroma not in CHROMAS:
            raise ValueError(f"chroma must be one of {sorted(CHROMAS)}, got {chroma!r}")
        ten = layout in deep.LAYOUTS
        self._rgb = "float16" if ten else "uint8"
        self._chroma = "replicate"
        super().__init__(device, size, layout, matrix, range, _lib.PIX_F16 if ten else _lib.PIX_U8, force_general)
        if chroma != "replicate":
            self.chroma = chroma

    def _tables(self):
        return (tables.rgb_matrix10 if self.layout in deep.LAYOUTS else tables.rgb_matrix)(self.matrix, self.range)

    def set_option(self, option: int, value: int) -> None:
        super().set_option(option, value)
        if int(option) == _lib.FIELD420_OPT_CHROMA:
            self._chroma = {number: name for name, number in CHROMAS.items()}[int(value)]

    @property
    def chroma(self) -> str:
        """"replicate", "left" or "center": how chroma is up-sampled inside a field (CRTFX_FIELD420_OPT_CHROMA)."""
        return self._chroma

    @chroma.setter
    def chroma(self, value: str) -> None:
        if value not in CHROMAS:
            raise ValueError(f"chroma must be one of {sorted(CHROMAS)}, got {value!r}")
        self.set_option(_lib.FIELD420_OPT_CHROMA, CHROMAS[value])


class EgressField420(EgressPlan):
    """plan = EgressField420(device, (h, w), layout, matrix="bt601", range="tv", chroma="center"); out = plan.run(frames[n, h, w, 3]) ->
    uint8[n, frame_bytes]; `frames` are uint8, or float16 on the 0..255 scale for "yuv420p10le" / "p010le".  h is a multiple of 4.  `frames`
    and `out` are tensors on `device` whose frames are contiguous (the batch stride is free; 10-bit: bases and strides must be even).
    `plan.chroma = "left"` switches a live plan.  The work is enqueued on the current stream of `device`; nothing synchronises."""
    _family, _force_option, _layouts = "egress_field420", _lib.EGRESS_FIELD420_OPT_FORCE_GENERAL, LAYOUTS
    _frame_bytes, _split_planes = frame_bytes, split_planes

    def __init__(self, device, size: Tuple[int, int], layout: str, matrix: str = "bt601", range: str = "tv", chroma: str = "center",    # noqa: A002
                 force_general: bool = False):
        if chroma not in EGRESS_CHROMAS:
            raise ValueError(f"chroma must be one of {sorted(EGRESS_CHROMAS)}, got {chroma!r}")
        ten = layout in deep.LAYOUTS
        self._rgb = "float16" if ten else "uint8"
        self._chroma = "center"
        super().__init__(device, size, layout, matrix, range, _lib.PIX_F16 if ten else _lib.PIX_U8, force_general)
        if chroma != "center":
            self.chroma = chroma

    def _tables(self):
        return (tables.yuv_matrix10 if self.layout in deep.LAYOUTS else tables.yuv_matrix)(self.matrix, self.range)

    def set_option(self, option: int, value: int) -> None:
        super().set_option(option, value)
        if int(option) == _lib.EGRESS_FIELD420_OPT_CHROMA:
            self._chroma = "left" if int(value) == _lib.EGRESS_FIELD420_LEFT else "center"

    @property
    def chroma(self) -> str:
        """"center" or "left": where a chroma sample sits inside its field (CRTFX_EGRESS_FIELD420_OPT_CHROMA)."""
        return self._chroma

    @chroma.setter
    def chroma(self, value: str) -> None:
        if value not in EGRESS_CHROMAS:
            raise ValueError(f"chroma must be one of {sorted(EGRESS_CHROMAS)}, got {value!r}")
        self.set_option(_lib.EGRESS_FIELD420_OPT_CHROMA, EGRESS_CHROMAS[value])
