"""The two ends of the effect chain as `cli.main` and `process_frames` wire them, on the current stream; the caller's events order the slots' reuse."""

from . import formats
from ._stage import resize_plan


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
    """Frames of `in_pix_fmt` at `src_hw`, staged at THEIR size: [source plan] (none for rgb24), RGB slots of src_hw, [resize] (ref:1039-1041)."""

    def __init__(self, device, render_hw, in_pix_fmt, in_matrix, in_range, in_chroma, src_hw, in_filter):
        import torch
        self.device, self.src_hw = device, tuple(src_hw)
        self.plan = formats.source_plan(device, self.src_hw, in_pix_fmt, in_matrix, in_range, in_chroma)
        self.resize = resize_plan(device, self.src_hw, render_hw, in_filter, torch.uint8) if self.src_hw != tuple(render_hw) else None
        self.frame_bytes = formats.frame_bytes(*self.src_hw, in_pix_fmt) if self.plan is None else self.plan.frame_bytes
        self.frame_shape = self.src_hw + (3,) if self.plan is None else (self.frame_bytes,)

    def slots(self, B: int, NS: int, pinned: bool = True):
        import torch
        shape = (B,) + self.frame_shape
        if self.plan is not None and self.resize is not None:
            self.rgb = [torch.empty((B,) + self.src_hw + (3,), dtype=torch.uint8, device=self.device) for _ in range(NS)]
        return self.adopt([torch.empty(shape, dtype=torch.uint8, device=self.device) for _ in range(NS)],
                          [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(NS)] if pinned else None)

    def convert(self, d: int, n: int, dst):
        rgb = self.dev[d][:n]
        if self.plan is not None:
            rgb = self.plan.run(rgb, out=dst if self.resize is None else self.rgb[d][:n])
        if self.resize is not None:
            self.resize.run(rgb, out=dst)


class DeliveryEnd:
    """Behind the chain: [the delivery resize] then [the egress plan, built for the delivery size].  `deliver` is None (as rendered) or a
    validated (dh, dw); `pix` is the chain's dtype.  Everything downstream is in frames of `frame_bytes`, batches of `shape(B)`."""

    def __init__(self, device, render_hw, pix, out_pix_fmt, out_matrix, out_range, out_chroma, deliver, deliver_filter):
        self.device, self.pix = device, pix
        self.size = tuple(deliver) if deliver is not None else tuple(render_hw)
        self.resize = resize_plan(device, render_hw, self.size, deliver_filter, pix) if deliver is not None else None
        self.egress = formats.egress_plan(device, self.size, out_pix_fmt, out_matrix, out_range, out_chroma)
        self.frame_bytes = self.size[0] * self.size[1] * 3 if self.egress is None else self.egress.frame_bytes

    def shape(self, B: int):
        return (B,) + self.size + (3,) if self.egress is None else (B, self.frame_bytes)

    def slots(self, dev_out):
        """(fin, send): what the egress plan reads and what is downloaded.  A missing stage costs no buffer: fin is dev_out, send is fin."""
        import torch
        B = int(dev_out[0].shape[0])
        self.out = self.fin = self.send = dev_out
        if self.resize is not None:
            self.fin = self.send = [torch.empty((B,) + self.size + (3,), dtype=self.pix, device=self.device) for _ in dev_out]
        if self.egress is not None:
            self.send = [torch.empty(self.shape(B), dtype=torch.uint8, device=self.device) for _ in dev_out]
        return self.fin, self.send

    def run(self, d: int, n: int):
        """Slot d's stages over its first n frames; returns the frames to download.  The caller has awaited the slot's last download."""
        if self.resize is not None:
            self.resize.run(self.out[d][:n], out=self.fin[d][:n])
        if self.egress is not None:
            self.egress.run(self.fin[d][:n], out=self.send[d][:n])
        return self.send[d][:n]
