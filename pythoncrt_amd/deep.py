"""`UnpackYuv10` and `EgressYuv10` — `UnpackYuv` and `EgressYuv` for a chain that runs on half pixels (FramePipeline(dtype=torch.float16)):
10-bit 4:2:0 frames as decoders hand them out and encoders take them — planar yuv420p10le (software) or semi-planar p010le (hardware), 3
bytes per pixel — become half RGB frames on the 0..255 scale in front of the chain, and its finished half frames become 10-bit 4:2:0 behind
it, several frames per launch (include/crtfx_deep.h holds the arithmetic and the two kernel paths of each direction).  The host builds the
integer matrices (tables.rgb_matrix10 / tables.yuv_matrix10); the library copies them.  Packed frames travel as uint8 tensors of
frame_bytes bytes, as the 8-bit stages' do: the 16-bit words are little-endian.  Not byte-equal to libswscale — see the header."""
from __future__ import annotations

from typing import Tuple

from . import _lib, tables
from ._stage import EgressPlan, SourcePlan

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
    """What the two plans share."""
    _layouts, _rgb, _split_planes = LAYOUTS, "float16", split_planes
    _frame_bytes = lambda h, w, layout: frame_bytes(h, w)     # noqa: E731

    def __init__(self, device, size: Tuple[int, int], layout: str = "yuv420p10le", matrix: str = "bt601", range: str = "tv",    # noqa: A002
                 pix_fmt: int = _lib.PIX_F16):
        super().__init__(device, size, layout, matrix, range, pix_fmt)


class UnpackYuv10(_Deep, SourcePlan):
    """plan = UnpackYuv10(device, (h, w), layout="yuv420p10le", matrix="bt601", range="tv"); rgb = plan.run(packed_u8[n, frame_bytes]) ->
    float16[n, h, w, 3] on the 0..255 scale.  `packed` and `out` are tensors on `device` whose frames are contiguous (the batch stride is
    free: slices of larger tensors are fine; bases and strides must be even).  The work is enqueued on the current stream of `device`;
    nothing synchronises."""
    _family, _force_option, _table = "unpack10", _lib.UNPACK10_OPT_FORCE_GENERAL, tables.rgb_matrix10


class EgressYuv10(_Deep, EgressPlan):
    """plan = EgressYuv10(device, (h, w), layout="yuv420p10le", matrix="bt601", range="tv"); out = plan.run(frames_f16[n, h, w, 3]) ->
    uint8[n, frame_bytes].  The rules of UnpackYuv10."""
    _family, _force_option, _table = "egress10", _lib.EGRESS10_OPT_FORCE_GENERAL, tables.yuv_matrix10
