"""`Signal` — the cable that fed the tube, on the device: every row of an RGB frame in HBM is encoded to an NTSC-like composite (or
S-Video) signal and decoded again (include/crtfx_signal.h), several frames per launch: colour that bleeds sideways, dot crawl on colour
edges, rainbow fringes on fine luma detail — what a second ffmpeg or shader pass in front of this project did.  One pixel is one sample at
4 x fsc — four times the colour subcarrier, about 754 samples to an active NTSC line — so feed SD-width sources (`in_size`); the resize
to the render size is behind the stage.  It stands directly behind the source plan, at the source's own size, in front of the
deinterlacer, the Canvas and the resize (ends.py, process_frames(in_signal=)).  `run` is the stateless call, `push` the one for a stream
of batches."""
from __future__ import annotations

from typing import Tuple

from . import _lib
from ._stage import FramePlan, pix_format

SIGNALS = ("composite", "svideo")
CHROMAS = ("sharp", "soft")


class Signal(FramePlan):
    """plan = Signal(device, (h, w), signal="composite", chroma="sharp", crawl=True, dtype=None);
    out = plan.run(frames[n, h, w, 3], index=0) -> [n, h, w, 3] of the same dtype: frame i is frame t = index + i of the stream, and the
    subcarrier's phase turns by 180 degrees per row and — with `crawl` — per frame, so only the parity of t matters.  "composite" adds
    chroma to luma and separates them with a notch (crosstalk: dot crawl and rainbows); "svideo" keeps them apart (only the chroma
    bandwidth is lost, and `crawl` changes nothing).  `chroma` is the decoder's chroma low-pass: "sharp" [1 2 3 4 3 2 1] / 16, "soft"
    [1 2 .. 8 .. 2 1] / 64.  One pixel is one sample at 4 x fsc, so feed SD-width frames; resize behind the stage.
    plan.push(frames) is run() at the plan's own counter, which it advances by n; plan.reset(index=0) sets the counter.  The C plan itself
    keeps nothing.  `dtype` is torch.uint8 (default) or torch.float16.  `frames` and `out` are tensors on `device` whose frames are
    contiguous (the batch stride is free: slices of larger tensors are fine).  The work is enqueued on the current stream of `device`;
    nothing synchronises.  plan.plan() is crtfx_signal_last_plan as a dictionary, e.g. {"signal": "k_signal<composite,soft,u8,vec>",
    "frames": "5"}.  Stated limits: NTSC-like only (no PAL, no burst-axis rotation, no RF noise); the rows of a woven interlaced frame
    are taken as consecutive lines; the chroma rows of a 4:2:0 source are formed in front of this stage by its source plan."""
    _family = "signal"
    _force_option = _lib.SIGNAL_OPT_FORCE_GENERAL

    def __init__(self, device, size: Tuple[int, int], signal: str = "composite", chroma: str = "sharp", crawl: bool = True, dtype=None,
                 force_general: bool = False):
        for name, value, allowed in (("signal", signal, SIGNALS), ("chroma", chroma, CHROMAS), ("crawl", crawl, (True, False))):
            if not any(value is a or (isinstance(a, str) and value == a) for a in allowed):
                raise ValueError(f"{name} must be one of {', '.join(str(a) for a in allowed)}, got {value!r}")
        self.signal, self.chroma, self.crawl = signal, chroma, crawl
        self._index = 0
        self._open(device)
        self.dtype, pix_fmt = pix_format(dtype)
        self.size = (int(size[0]), int(size[1]))
        self._create(self.size[0], self.size[1], pix_fmt, SIGNALS.index(signal), CHROMAS.index(chroma), int(crawl))
        self._frames(self.size + (self.dtype,))
        if force_general:
            self.force_general = True

    def run(self, frames, out=None, index: int = 0):
        n = self._check_frames(frames)
        if isinstance(index, bool) or not isinstance(index, int) or index < 0:
            raise ValueError(f"index must be a non-negative integer, got {index!r}")
        return self._run(frames, self._check_out(n, out), n, index)

    def push(self, frames, out=None):
        """run() at the plan's counter, which advances by the frames pushed."""
        out = self.run(frames, out, self._index)
        self._index += int(frames.shape[0])
        return out

    def reset(self, index: int = 0) -> None:
        """Set the counter: the next frame pushed is frame `index` of its stream."""
        if isinstance(index, bool) or not isinstance(index, int) or index < 0:
            raise ValueError(f"index must be a non-negative integer, got {index!r}")
        self._index = index
