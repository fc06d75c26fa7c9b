"""The one registry of the pixel formats a source or egress stage exists for: format name -> family.  `process_frames` and the CLI pick
their plans, their frame sizes and the names they accept from here; a new format is a new entry ("rgb24", the chain's own format, needs
no stage and is no entry)."""
from __future__ import annotations

from typing import Callable, NamedTuple, Tuple

from . import deep, deep444, egress, field420, sited, unpack, yuv422


class Family(NamedTuple):
    names: Tuple[str, ...]      # the formats of the family, as ffmpeg spells them
    source: type                # the plan in front of the chain: source(device, (h, w), layout=name, matrix=, range=)
    egress: type                # the plan behind it, same signature
    frame_bytes: Callable       # (h, w, name) -> bytes of one packed frame
    bits: int                   # 8: the chain between runs on uint8 pixels; 10: on half pixels


YUV420 = Family(tuple(egress.LAYOUTS), unpack.UnpackYuv, egress.EgressYuv, lambda h, w, fmt: egress.frame_bytes(h, w), 8)
YUV422 = Family(tuple(yuv422.LAYOUTS), yuv422.UnpackYuv422, yuv422.EgressYuv422, yuv422.frame_bytes, 8)
DEEP420 = Family(tuple(deep.LAYOUTS), deep.UnpackYuv10, deep.EgressYuv10, lambda h, w, fmt: deep.frame_bytes(h, w), 10)
DEEP444 = Family(tuple(deep444.FORMATS), deep444.UnpackDeep444, deep444.EgressDeep444, deep444.frame_bytes, 10)

FORMATS = {name: family for family in (YUV420, YUV422, DEEP420, DEEP444) for name in family.names}
PIX_FMTS = ("rgb24",) + tuple(FORMATS)          # what in_pix_fmt / out_pix_fmt, --in-pix-fmt / --out-pix-fmt accept


def bits(fmt: str) -> int:
    """8 or 10: the sample depth of `fmt` (a member of PIX_FMTS), which decides what the chain runs on."""
    return FORMATS[fmt].bits if fmt in FORMATS else 8


def frame_bytes(h: int, w: int, fmt: str) -> int:
    """Bytes of one packed h x w frame of `fmt` (a member of PIX_FMTS), rows unpadded."""
    return FORMATS[fmt].frame_bytes(int(h), int(w), fmt) if fmt in FORMATS else int(h) * int(w) * 3


def source_plan(device, size, fmt: str, matrix: str, range: str, chroma: str, rows: str = "progressive"):     # noqa: A002 - the stages' keyword
    """The plan in front of the chain: None for "rgb24", the family's source under chroma "replicate", else UnpackSited at that siting.
    With rows "interlaced" (a 4:2:0 format whose chroma rows alternate between the fields): UnpackField420 at that chroma."""
    if fmt == "rgb24":
        return None
    if rows == "interlaced":
        return field420.UnpackField420(device, size, layout=fmt, matrix=matrix, range=range, chroma=chroma)
    cls, siting = (FORMATS[fmt].source, {}) if chroma == "replicate" else (sited.UnpackSited, {"siting": chroma})
    return cls(device, size, layout=fmt, matrix=matrix, range=range, **siting)


def egress_plan(device, size, fmt: str, matrix: str, range: str, chroma: str, rows: str = "progressive"):     # noqa: A002
    """The plan behind the chain: None for "rgb24", the family's egress under chroma "center" (the box mean), else EgressSited at "left".
    With rows "interlaced" (a 4:2:0 format whose chroma rows alternate between the fields): EgressField420 at that chroma."""
    if fmt == "rgb24":
        return None
    if rows == "interlaced":
        return field420.EgressField420(device, size, layout=fmt, matrix=matrix, range=range, chroma=chroma)
    cls, siting = (FORMATS[fmt].egress, {}) if chroma == "center" else (sited.EgressSited, {"siting": chroma})
    return cls(device, size, layout=fmt, matrix=matrix, range=range, **siting)
