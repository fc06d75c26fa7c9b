"""The two ends of the effect chain as `cli.main` and `process_frames` wire them, on the current stream; the caller's events order the slots' reuse."""

from . import formats
from ._stage import resize_plan
from .adeint import METHOD as ADAPTIVE, AdaptiveDeinterlace
from .canvas import Canvas, fit_crop, fit_pad
from .deint import Deinterlace
from .depth import Narrow, Widen
from .interlace import Interlace
from .lut3d import Lut3D
from .pal import PalSignal
from .signal import Signal


def depth_stages(in_pix_fmt: str, out_pix_fmt: str, chain_pix: str = "auto", dither: str = "none"):
    """(half, widen, narrow) for a pair of formats the caller has admitted: does the chain run on half pixels, does a Widen stand behind
    the source's uint8 stages, and the dither of the Narrow in front of the 8-bit delivery (None: there is none).  Under "auto" the chain
    is half between two 10-bit ends and neither depth stage exists; under "half" every 8-bit (or rgb24) end gets its depth stage."""
    deep_in, deep_out, forced = formats.bits(in_pix_fmt) == 10, formats.bits(out_pix_fmt) == 10, chain_pix == "half"
    return forced or (deep_in and deep_out), forced and not deep_in, dither if forced and not deep_out else None


class StagingSlots:
    """Slots in front of the chain: per slot a uint8 device tensor, the pinned host tensor it is uploaded from (None: the caller stages on the
    host itself, as the CLI's reader does) and the two events that order their reuse.  On its own: slots that ARE the chain's input."""

    def adopt(self, dev, pin=None):
        self.dev, self.pin = dev, pin
        self.np = [t.numpy() for t in pin] if pin is not None else None
        self.up_done = [None] * len(dev)             # the upload that last read pin[d]
        self.kernels_done = [None] * len(dev)        # the kernels that last read dev[d] (and, on the same stream, what convert() ran behind them)
        return self

    def convert(self, d: int, n: int, dst):
        pass                                         # nothing stands between these slots and the chain


class SourceEnd(StagingSlots):
    """Frames of `in_pix_fmt` at `src_hw`, staged at THEIR size: [source plan] (none for rgb24), RGB slots of src_hw, [Canvas cutting the
    window `crop` = (y, x, ch, cw) of the source frame], [resize of what is left to the render size] (ref:1039-1041).  The RGB side of the
    source plan, the window and the resize are frames of `dtype`.  With `widen` those are uint8 frames in front of a half chain: a Widen at
    the render size (include/crtfx_depth.h) is then the last stage and writes the chain's half input — for an rgb24 frame at render size
    the only one.  `deinterlace` = (method, order, fields) puts a Deinterlace (include/crtfx_deint.h) directly behind the source plan, at
    src_hw and on `dtype`, in front of the Canvas and the resize: a crop at an odd y, or any resize, would mix the fields; with the method
    "adaptive" an AdaptiveDeinterlace (include/crtfx_adeint.h) stands there instead, convert() pushes each batch behind the one before it,
    and restart() starts a new history (the frames that follow are not the continuation of those converted before).  `ratio` is the
    frames it writes per source frame (1 without it): the staged slots hold SOURCE frames and convert(d, n, dst) writes n * ratio frames.
    `lut` is None or a Cube: a Lut3D (include/crtfx_lut3d.h) at the render size and on the CHAIN's pixel type is then the last stage,
    behind the resize and behind the Widen, and writes the chain's input — for an rgb24 frame at render size the only one.
    `signal` is None or (signal, chroma, crawl): a Signal (include/crtfx_signal.h) then stands directly behind the source plan, at src_hw
    and on `dtype`, in front of the Deinterlace, the Canvas, the resize, the Widen and the Lut3D — the cable carried the fields and the
    source's own samples, one pixel being one sample at four times the colour subcarrier — for an rgb24 frame at render size the only
    stage.  Its frame index t is the source frame's index in the stream: the caller sets `index` to that of the batch's first frame
    before convert() (0 until it does); several ends of one stream (a mixed-size rgb24 source) are each told.
    `pal` is None or (decoder, phase): with a `signal`, a PalSignal (include/crtfx_pal.h) of those two values then stands in the Signal's
    place — same size, sample type and index; it is `signal` too.
    `chroma_rows` says which luma rows a chroma row of a 4:2:0 source belongs to: "progressive" — rows 2c and 2c + 1, one of each field: in
    front of a Deinterlace, a Signal or a probe the colour of the two fields is then already mixed — or "interlaced" — the rows of its own
    field, as an interlaced encoder sub-samples them: the source plan is then an UnpackField420 (include/crtfx_field420.h) at `in_chroma`,
    and the stages behind it read fields whose colour is their own."""

    def __init__(self, device, render_hw, in_pix_fmt, in_matrix, in_range, in_chroma, src_hw, in_filter, crop=None, dtype=None, widen=False,
                 deinterlace=None, lut=None, signal=None, chroma_rows="progressive", pal=None):
        import torch
        self.device, self.src_hw = device, tuple(src_hw)
        self.dtype = torch.uint8 if dtype is None or widen else dtype      # widen: `dtype` is the chain's, the stages in front of it run on uint8
        self.plan = formats.source_plan(device, self.src_hw, in_pix_fmt, in_matrix, in_range, in_chroma,
                                        *(() if chroma_rows == "progressive" else (chroma_rows,)))
        self.signal, self.index = None, 0
        if signal is not None and pal is not None:
            self.signal = PalSignal(device, self.src_hw, signal=signal[0], chroma=signal[1], crawl=signal[2], decoder=pal[0], phase=pal[1], dtype=self.dtype)
        elif signal is not None:
            self.signal = Signal(device, self.src_hw, signal=signal[0], chroma=signal[1], crawl=signal[2], dtype=self.dtype)
        self.deint, self.ratio, self.adaptive = None, 1, False
        if deinterlace is not None:
            method, order, fields = deinterlace
            self.adaptive = method == ADAPTIVE
            self.deint = (AdaptiveDeinterlace(device, self.src_hw, order=order, fields=fields, dtype=self.dtype) if self.adaptive else
                          Deinterlace(device, self.src_hw, method=method, order=order, fields=fields, dtype=self.dtype))
            self.ratio = 2 if fields == "both" else 1
        self.canvas, cut = None, self.src_hw
        if crop is not None:
            cut = (int(crop[2]), int(crop[3]))
            self.canvas = Canvas(device, self.src_hw, cut, window=tuple(int(v) for v in crop), dtype=self.dtype)
        self.resize = resize_plan(device, cut, render_hw, in_filter, self.dtype) if cut != tuple(render_hw) else None
        self.widen = Widen(device, tuple(render_hw)) if widen else None
        self.chain_dtype = dtype if widen else self.dtype                  # what the last stage writes
        self.lut = Lut3D(device, tuple(render_hw), lut, dtype=self.chain_dtype) if lut is not None else None
        self.frame_bytes = formats.frame_bytes(*self.src_hw, in_pix_fmt) if self.plan is None else self.plan.frame_bytes
        self.frame_shape = self.src_hw + (3,) if self.plan is None else (self.frame_bytes,)
        # the stages present, each with the size of the RGB frames it writes; the last one writes the chain's input
        self.stages = [(st, hw) for st, hw in ((self.plan, self.src_hw), (self.signal, self.src_hw), (self.deint, self.src_hw), (self.canvas, cut),
                                                    (self.resize, tuple(render_hw)), (self.widen, tuple(render_hw)),
                                                    (self.lut, tuple(render_hw))) if st is not None]

    def slots(self, B: int, NS: int, pinned: bool = True):
        import torch
        shape = (B,) + self.frame_shape
        # a stage that is not the last one writes RGB slots of its own: a missing stage costs no buffer.  B counts source frames: the
        # Deinterlace and every stage behind it write B * ratio frames
        behind = [any(st is self.deint for st, _ in self.stages[:i + 1]) for i in range(len(self.stages))]
        self.mid = [[torch.empty((B * (self.ratio if behind[i] else 1),) + hw + (3,), dtype=self.chain_dtype if st is self.widen else self.dtype,
                                 device=self.device) for _ in range(NS)]
                    for i, (st, hw) in enumerate(self.stages[:-1])]
        return self.adopt([torch.empty(shape, dtype=torch.uint8, device=self.device) for _ in range(NS)],
                          [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(NS)] if pinned else None)

    def convert(self, d: int, n: int, dst):
        x = self.dev[d][:n]
        for i, (stage, _) in enumerate(self.stages):
            if stage is self.deint:
                n *= self.ratio
            run = stage.push if self.adaptive and stage is self.deint else stage.run      # the adaptive plan keeps the last frame of the batch before
            x = run(x, out=dst if i == len(self.stages) - 1 else self.mid[i][d][:n], **({"index": self.index} if stage is self.signal else {}))

    def restart(self):
        """The next batch converted does not continue the one before it: an AdaptiveDeinterlace forgets its kept frame.  Nothing otherwise."""
        if self.adaptive:
            self.deint.reset()


class DeliveryEnd:
    """Behind the chain: [the delivery geometry: a resize, a Canvas, or both] then [the egress plan, built for the delivery size].
    `deliver` is None (as rendered) or a validated (dh, dw); `pix` is the chain's dtype.  `deliver_fit` says how a render of another aspect
    meets the delivery: "stretch" resizes it to (dh, dw); "pad" resizes it to fit_pad's inner size (no resize where that is the render
    size) and a Canvas centres that on a (dh, dw) frame of `pad_color`; "crop" has a Canvas cut fit_crop's window and resizes that to
    (dh, dw) (no resize where the window has that size).  Where the aspects agree — inner = delivery, window = the whole render — no
    Canvas is built and the stages are those of "stretch".  `narrow` is None or a dither name of depth.DITHERS: the chain runs on half
    pixels and the delivery is an 8-bit one, so behind the geometry, which runs on the half frames, a Narrow at the delivery size
    (include/crtfx_depth.h) writes the uint8 frames the egress plan reads — or, for "rgb24", the frames that are downloaded; the dither's
    coordinates are those of the delivered frame.  `lut` is None or a Cube: a Lut3D (include/crtfx_lut3d.h) at the render size and on
    `pix` is then the FIRST stage, in front of the delivery resize, the Canvas, the Narrow and the egress plan — a pad colour is not
    transformed and the dither stays last.  `interlace` is None or (order, lowpass): an Interlace (include/crtfx_interlace.h) at the
    DELIVERY size and on `pix` then stands behind the delivery resize and the Canvas — a vertical resize would mix the fields — and in front
    of the Narrow and the egress plan: the low-pass runs at the chain's precision, the dither's coordinates are those of the delivered
    frame and the dither stays last.  It weaves two finished frames into one, an odd last frame of a run with itself: from it on every
    buffer holds `frames(B)` = ceil(B / 2) frames, and run(d, m) returns frames(m).  `chroma_rows` says which luma rows a chroma row of a
    4:2:0 delivery is formed from: "progressive" — rows 2c and 2c + 1, one of each field, as the family's egress plan and EgressSited form
    it — or "interlaced" — rows of the chroma row's own field only (EgressField420, include/crtfx_egress_field420.h; the delivered height
    is a multiple of 4), as an interlaced decoder reads a woven frame; 4:2:2, 4:4:4 and rgb24 deliveries have no such pairing.  Everything
    downstream is in frames of `frame_bytes`, batches of `shape(frames(B))`."""

    def __init__(self, device, render_hw, pix, out_pix_fmt, out_matrix, out_range, out_chroma, deliver, deliver_filter,
                 deliver_fit="stretch", pad_color=(0, 0, 0), narrow=None, lut=None, interlace=None, chroma_rows="progressive"):
        self.device, self.pix = device, pix
        self.size = tuple(deliver) if deliver is not None else tuple(render_hw)
        self.resize = self.canvas = self.narrow = self.lut = self.interlace = None
        self.stages = []                 # (plan, the size of the frames it writes), in order, in front of the egress plan
        if lut is not None:
            self.lut = Lut3D(device, tuple(render_hw), lut, dtype=pix)
            self.stages.append((self.lut, tuple(render_hw)))
        inner, at = fit_pad(render_hw, self.size) if deliver is not None and deliver_fit == "pad" else (self.size, (0, 0))
        window = fit_crop(render_hw, self.size) if deliver is not None and deliver_fit == "crop" else (0, 0) + tuple(render_hw)
        if inner != self.size:
            if inner != tuple(render_hw):
                self.resize = resize_plan(device, render_hw, inner, deliver_filter, pix)
                self.stages.append((self.resize, inner))
            self.canvas = Canvas(device, inner, self.size, at=at, fill=pad_color, dtype=pix)
            self.stages.append((self.canvas, self.size))
        elif window[2:] != tuple(render_hw):
            self.canvas = Canvas(device, render_hw, window[2:], window=window, dtype=pix)
            self.stages.append((self.canvas, window[2:]))
            if window[2:] != self.size:
                self.resize = resize_plan(device, window[2:], self.size, deliver_filter, pix)
                self.stages.append((self.resize, self.size))
        elif deliver is not None:
            self.resize = resize_plan(device, render_hw, self.size, deliver_filter, pix)
            self.stages.append((self.resize, self.size))
        if interlace is not None:
            self.interlace = Interlace(device, self.size, order=interlace[0], lowpass=interlace[1], dtype=pix)
            self.stages.append((self.interlace, self.size))
        if narrow is not None:
            self.narrow = Narrow(device, self.size, dither=narrow)
            self.stages.append((self.narrow, self.size))
        self.egress = formats.egress_plan(device, self.size, out_pix_fmt, out_matrix, out_range, out_chroma,
                                          *(() if chroma_rows == "progressive" else (chroma_rows,)))
        self.frame_bytes = self.size[0] * self.size[1] * 3 if self.egress is None else self.egress.frame_bytes

    def frames(self, m: int) -> int:
        """The frames delivered for m frames of the chain: m, or ceil(m / 2) behind an Interlace."""
        return m if self.interlace is None else -(-m // self.interlace.frames_in)

    def shape(self, B: int):
        """Of a batch of B DELIVERED frames (frames(the chain's batch))."""
        return (B,) + self.size + (3,) if self.egress is None else (B, self.frame_bytes)

    def slots(self, dev_out):
        """(fin, send): what the egress plan reads and what is downloaded.  A missing stage costs no buffer: fin is dev_out, send is fin."""
        import torch
        B = int(dev_out[0].shape[0])
        self.out = self.fin = self.send = dev_out
        # the Interlace and every stage behind it write frames(B) frames
        behind = [any(st is self.interlace for st, _ in self.stages[:i + 1]) for i in range(len(self.stages))]
        self.bufs = [[torch.empty((self.frames(B) if behind[i] else B,) + hw + (3,), dtype=torch.uint8 if st is self.narrow else self.pix,
                                  device=self.device) for _ in dev_out]
                     for i, (st, hw) in enumerate(self.stages)]
        if self.bufs:
            self.fin = self.send = self.bufs[-1]
        if self.egress is not None:
            self.send = [torch.empty(self.shape(self.frames(B)), dtype=torch.uint8, device=self.device) for _ in dev_out]
        return self.fin, self.send

    def run(self, d: int, n: int):
        """Slot d's stages over its first n frames; returns the frames to download, frames(n) of them.  The caller has awaited the slot's
        last download."""
        x = self.out[d][:n]
        for (stage, _), buf in zip(self.stages, self.bufs):
            if stage is self.interlace:
                n = self.frames(n)
            x = stage.run(x, out=buf[d][:n])
        if self.egress is not None:
            self.egress.run(self.fin[d][:n], out=self.send[d][:n])
        return self.send[d][:n]
