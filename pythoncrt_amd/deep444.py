"""`UnpackDeep444` and `EgressDeep444` — `UnpackYuv10` and `EgressYuv10` for full-resolution deep colour: yuv444p10le (ProRes 4444 /
DNxHR 444 decodes), gbrp10le (DPX / TIFF / EXR sequences through ffmpeg) and x2rgb10le (10-bit screen and KMS capture).  In front of a
chain that runs on half pixels (FramePipeline(dtype=torch.float16)) such frames become half RGB frames on the 0..255 scale, behind it the
finished half frames become 10-bit 4:4:4 again, several frames per launch (include/crtfx_444.h holds the two memory layouts, the
arithmetic and the two kernel paths of each direction).  The three formats differ only in layout and table: yuv444p10le takes
tables.rgb_matrix10 / tables.yuv_matrix10 with the `matrix` and `range` keywords; for gbrp10le and x2rgb10le, which are full-range RGB
(tables.rgb_scale10), those two keywords do not apply and are ignored.  Packed frames travel as uint8 tensors of frame_bytes bytes: the
16-bit and 32-bit words are little-endian.  Not byte-equal to libswscale — see the header."""
from __future__ import annotations

from typing import Tuple

from . import _lib, tables
from ._stage import EgressPlan, SourcePlan

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
    """What the two plans share: `layout` is the format name, and the table follows it."""
    _layouts, _layout_word, _rgb, _split_planes, _frame_bytes = FORMATS, "the format", "float16", split_planes, frame_bytes
    _egress = 0

    def __init__(self, device, size: Tuple[int, int], layout: str = "yuv444p10le", matrix: str = "bt601", range: str = "tv",    # noqa: A002
                 pix_fmt: int = _lib.PIX_F16):
        super().__init__(device, size, layout, matrix, range, pix_fmt)

    def _tables(self):
        if self.layout in _RGB_ORDER:            # full-range RGB: `matrix` and `range` do not apply
            return tables.rgb_scale10(_RGB_ORDER[self.layout])[self._egress]
        return (tables.yuv_matrix10 if self._egress else tables.rgb_matrix10)(self.matrix, self.range)


class UnpackDeep444(_Deep444, SourcePlan):
    """plan = UnpackDeep444(device, (h, w), layout="yuv444p10le", matrix="bt601", range="tv"); rgb = plan.run(packed_u8[n, frame_bytes]) ->
    float16[n, h, w, 3] on the 0..255 scale.  `layout` is the format name: "yuv444p10le", "gbrp10le" or "x2rgb10le"; `matrix` and `range`
    apply to yuv444p10le only.  `packed` and `out` are tensors on `device` whose frames are contiguous (the batch stride is free: slices
    of larger tensors are fine; bases and strides must be even, and multiples of 4 on the x2rgb10le side).  The work is enqueued on the
    current stream of `device`; nothing synchronises."""
    _family, _force_option, _egress = "unpack444", _lib.UNPACK444_OPT_FORCE_GENERAL, 0


class EgressDeep444(_Deep444, EgressPlan):
    """plan = EgressDeep444(device, (h, w), layout="yuv444p10le", matrix="bt601", range="tv"); out = plan.run(frames_f16[n, h, w, 3]) ->
    uint8[n, frame_bytes].  The rules of UnpackDeep444."""
    _family, _force_option, _egress = "egress444", _lib.EGRESS444_OPT_FORCE_GENERAL, 1
