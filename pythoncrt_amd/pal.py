"""`PalSignal` — the cable of 576i sources, on the device: every row of an RGB frame in HBM is encoded to a PAL-like composite (or S-Video)
signal and decoded again by a decoder with a phase error and a one-line delay line (include/crtfx_pal.h), several frames per launch.  The
subcarrier turns 270 degrees per line and per frame and the V axis switches sign every line: with the delay line a phase error
desaturates the picture instead of turning its hue and vertical chroma detail is halved; without it ("simple") a phase error shows as
Hanover bars.  One pixel is one sample at 4 x fsc — four times the colour subcarrier — so feed SD-width sources (`in_size`); the resize to
the render size is behind the stage.  It stands where `Signal` stands (signal.py, whose NTSC family is untouched and has no phase knob):
directly behind the source plan, at the source's own size (ends.py, process_frames(in_signal=, signal_standard="pal")).  `run` is the
stateless call, `push` the one for a stream of batches."""
from __future__ import annotations

from typing import Tuple

from . import _lib
from ._stage import FramePlan, pix_format
from .signal import CHROMAS, SIGNALS

DECODERS = ("delay", "simple")
PHASES = (-180, 180)                    # the decoder's phase error, whole degrees, both ends included
STRIP = 8                               # rows of a vec wave's strip (include/crtfx_pal.h)


def check_phase(phase, name="phase"):
    if isinstance(phase, bool) or not isinstance(phase, int) or not PHASES[0] <= phase <= PHASES[1]:
        raise ValueError(f"{name} must be an integer number of degrees in {PHASES[0]}..{PHASES[1]}, got {phase!r}")
    return phase


def phase_table(degrees: int) -> Tuple[int, int]:
    """(llrint(4096 cos theta), llrint(4096 sin theta)) as the library computes them (crtfx_pal_phase_table; no device is needed)."""
    import ctypes
    c, s = ctypes.c_int(), ctypes.c_int()
    if _lib.load().crtfx_pal_phase_table(int(degrees), ctypes.byref(c), ctypes.byref(s)) != _lib.OK:
        raise ValueError(f"phase must be an integer number of degrees in {PHASES[0]}..{PHASES[1]}, got {degrees!r}")
    return c.value, s.value


class PalSignal(FramePlan):
    """plan = PalSignal(device, (h, w), signal="composite", chroma="sharp", crawl=True, decoder="delay", phase=0, dtype=None);
    out = plan.run(frames[n, h, w, 3], index=0) -> [n, h, w, 3] of the same dtype: frame i is frame t = index + i of the stream, and the
    subcarrier's phase turns by 270 degrees per row and — with `crawl` — per frame, so only t mod 4 matters.  "composite" adds chroma to
    luma and separates them with a notch; "svideo" keeps them apart.  `chroma` is the decoder's chroma low-pass: "sharp"
    [1 2 3 4 3 2 1] / 16, "soft" [1 2 .. 8 .. 2 1] / 64.  `decoder` is "delay" — every row's chroma is averaged with the row above, row 0
    with row 1 — or "simple".  `phase` is the decoder's phase error in whole degrees, -180..180: under "delay" the picture loses
    saturation by cos(phase), under "simple" even and odd rows turn their hue opposite ways.  One pixel is one sample at 4 x fsc, so feed
    SD-width frames; resize behind the stage.
    plan.push(frames) is run() at the plan's own counter, which it advances by n; plan.reset(index=0) sets the counter.  The C plan itself
    keeps nothing.  `dtype` is torch.uint8 (default) or torch.float16.  `frames` and `out` are tensors on `device` whose frames are
    contiguous (the batch stride is free: slices of larger tensors are fine).  The work is enqueued on the current stream of `device`;
    nothing synchronises.  plan.plan() is crtfx_pal_last_plan as a dictionary, e.g. {"pal": "k_pal<composite,soft,delay,u8,vec>",
    "frames": "5"}.  Stated limits: the rows of a woven interlaced frame are taken as consecutive lines; no 25 Hz offset; no RF noise;
    the chroma rows of a 4:2:0 source are formed in front of this stage by its source plan."""
    _family = "pal"
    _force_option = _lib.PAL_OPT_FORCE_GENERAL

    def __init__(self, device, size: Tuple[int, int], signal: str = "composite", chroma: str = "sharp", crawl: bool = True,
                 decoder: str = "delay", phase: int = 0, dtype=None, force_general: bool = False):
        for name, value, allowed in (("signal", signal, SIGNALS), ("chroma", chroma, CHROMAS), ("crawl", crawl, (True, False)),
                                     ("decoder", decoder, DECODERS)):
            if not any(value is a or (isinstance(a, str) and value == a) for a in allowed):
                raise ValueError(f"{name} must be one of {', '.join(str(a) for a in allowed)}, got {value!r}")
        check_phase(phase)
        self.signal, self.chroma, self.crawl, self.decoder, self.phase = signal, chroma, crawl, decoder, phase
        self._index = 0
        self._open(device)
        self.dtype, pix_fmt = pix_format(dtype)
        self.size = (int(size[0]), int(size[1]))
        self._create(self.size[0], self.size[1], pix_fmt, SIGNALS.index(signal), CHROMAS.index(chroma), int(crawl), DECODERS.index(decoder), phase)
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
