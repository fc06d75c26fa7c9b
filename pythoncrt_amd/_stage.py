"""What every plan object over a libcrtfx handle shares.  `Handle` is the handle of one crtfx_<family>_* family behind a plan object: device,
create and its error path, options, the batched run, the plan string, close.  On it stand `StagePlan` — the ten format-stage plans
(unpack.py, egress.py, deep.py, yuv422.py, deep444.py), the two sited plans (sited.py: source and egress) and the two field-paired 4:2:0
plans (field420.py: source and egress), seven entry points each
(`_lib.stage_symbols`) — `ResizePlan` — the three resize plans (ingest.py, resize16.py, resample.py), six entry points each
(`_lib.resize_symbols`) — and `FramePlan` — the ten plans of the nine frame stages (canvas.py, depth.py, deint.py, adeint.py, lut3d.py, interlace.py, signal.py, pal.py, probe.py), six
entry points and a create of its own each (`_lib.frame_symbols`).  A family module declares short classes on `SourcePlan` / `EgressPlan` /
`ResizePlan` / `FramePlan` — family name, C layout numbers or dtype, table function, frame size, its own arguments — and keeps what is truly
its own; everything else is here."""
from __future__ import annotations

import ctypes

from . import _lib, tables


class Handle:
    """The handle of one crtfx_<family>_* family.  Frames are tensors on `device` whose frames are contiguous (the batch stride is free:
    slices of larger tensors are fine).  The work is enqueued on the current stream of `device`; nothing synchronises."""
    _family = ""                 # crtfx_<family>_*
    _force_option = 1            # the family's *_OPT_FORCE_GENERAL

    def _open(self, device):
        """The library and the device the plan lives on: what comes before the family's own argument checks."""
        import torch
        self.lib = _lib.load()
        self._fn = lambda name: getattr(self.lib, f"crtfx_{self._family}_{name}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"{type(self).__name__} needs a ROCm device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())

    def _create(self, *args):
        """crtfx_<family>_create(device, *args, &plan)."""
        self._plan = ctypes.c_void_p()
        rc = self._fn("create")(self.device.index, *args, ctypes.byref(self._plan))
        if rc != _lib.OK:
            self._plan = None
            raise _lib.CrtfxError(rc, (self._fn("last_error")(None) or b"").decode())
        self._force_general = False

    def _check(self, rc):
        if rc != _lib.OK:
            raise _lib.CrtfxError(rc, (self._fn("last_error")(self._plan) or b"").decode())

    def set_option(self, option: int, value: int) -> None:
        """Testing / A-B switches of crtfx_<family>_set_option, e.g. set_option(_lib.UNPACK_OPT_FORCE_GENERAL, 1)."""
        self._check(self._fn("set_option")(self._plan, int(option), int(value)))
        if int(option) == self._force_option:
            self._force_general = bool(value)

    @property
    def force_general(self) -> bool:
        """Take the general kernel whatever the width and alignment (*_OPT_FORCE_GENERAL)."""
        return self._force_general

    @force_general.setter
    def force_general(self, value) -> None:
        self.set_option(self._force_option, 1 if value else 0)

    def _run(self, src, dst, n, *first):
        """crtfx_<family>_run(plan, *first, src, its stride, dst, its stride, n, stream)."""
        import torch
        for name, t in (("input", src), ("out", dst)):
            if n and not t[0].is_contiguous():
                raise ValueError(f"every frame of the {name} must be contiguous (only the batch stride is free)")
        if n == 0:
            return dst
        with torch.cuda.device(self.device):
            self._check(self._fn("run")(self._plan, *first, src.data_ptr(), src.stride(0) * src.element_size(), dst.data_ptr(),
                                        dst.stride(0) * dst.element_size(), n, torch.cuda.current_stream(self.device).cuda_stream))
        return dst

    def __call__(self, src, out=None):
        return self.run(src, out)

    def last_plan(self) -> str:
        """crtfx_<family>_last_plan, e.g. "unpack422=k_unpack_422<uyvy422,vec>;frames=5"."""
        buf = ctypes.create_string_buffer(256)
        self._check(self._fn("last_plan")(self._plan, buf, len(buf)))
        return buf.value.decode()

    def plan(self) -> dict:
        """last_plan() as a dictionary, e.g. {"unpack422": "k_unpack_422<uyvy422,vec>", "frames": "5"}."""
        return dict(kv.split("=", 1) for kv in self.last_plan().split(";") if kv)

    def close(self) -> None:
        if getattr(self, "_plan", None):
            self._fn("destroy")(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 - interpreter shutdown
            pass


class StagePlan(Handle):
    """A format stage.  `packed` frames are uint8 [n, frame_bytes]; RGB frames are `_rgb` [n, h, w, 3]."""
    _layouts = {}                # layout name -> the C layout number
    _layout_word = "layout"      # what the family calls a member of _layouts
    _rgb = "uint8"               # torch dtype of the RGB side: "uint8" or "float16"
    _table = None                # (matrix, range) -> (m, off): a tables.* function
    _frame_bytes = None          # (h, w, layout) -> bytes of one packed frame
    _split_planes = None         # the family module's split_planes

    def __init__(self, device, size, layout, matrix, range, pix_fmt, force_general=False):     # noqa: A002 - the stages' keyword
        self._open(device)
        if layout not in self._layouts:
            raise ValueError(f"{self._layout_word} must be one of {sorted(self._layouts)}, got {layout!r}")
        self.size = (int(size[0]), int(size[1]))
        self.layout, self.matrix, self.range = layout, matrix, range
        if min(self.size) < 1:
            raise _lib.CrtfxError(_lib.E_INVALID, f"size {self.size} must be at least 1 x 1")
        m, off = self._tables()
        self.frame_bytes = type(self)._frame_bytes(self.size[0], self.size[1], layout)
        self._create(self.size[0], self.size[1], int(pix_fmt), self._layouts[layout], tables.ptr(m), tables.ptr(off))
        assert self._fn("frame_bytes")(self._plan) == self.frame_bytes
        if force_general:
            self.force_general = True

    def _tables(self):
        return type(self)._table(self.matrix, self.range)

    def _rgb_dtype(self):
        import torch
        return getattr(torch, self._rgb)

    def planes(self, packed):
        """Views of `packed` ([n, frame_bytes] or [frame_bytes]; a tensor or a numpy array) — see the family module's split_planes."""
        return type(self)._split_planes(packed, self.size, self.layout)


class SourcePlan(StagePlan):
    """In front of the chain: rgb = plan.run(packed_u8[n, frame_bytes]) -> `_rgb`[n, h, w, 3] (plan(packed) is the same call)."""

    def run(self, packed, out=None):
        import torch
        h, w = self.size
        rgb = self._rgb_dtype()
        if packed.dtype != torch.uint8:
            raise _lib.CrtfxError(_lib.E_UNSUPPORTED, f"packed {self.layout} frames are uint8 tensors of frame_bytes bytes, got {packed.dtype}")
        if packed.dim() != 2 or int(packed.shape[1]) != self.frame_bytes or packed.device != self.device:
            raise ValueError(f"packed must be uint8 [n, {self.frame_bytes}] on {self.device}, got {tuple(packed.shape)} on {packed.device}")
        n = int(packed.shape[0])
        if out is None:
            out = torch.empty((n, h, w, 3), dtype=rgb, device=self.device)
        if out.dtype != rgb or tuple(out.shape) != (n, h, w, 3) or out.device != self.device:
            raise ValueError(f"out must be {self._rgb} [{n}, {h}, {w}, 3] on {self.device}")
        return self._run(packed, out, n)


class EgressPlan(StagePlan):
    """Behind the chain: out = plan.run(frames[n, h, w, 3] of `_rgb`) -> uint8[n, frame_bytes] (plan(frames) is the same call)."""

    def run(self, frames, out=None):
        import torch
        h, w = self.size
        rgb = self._rgb_dtype()
        if frames.dtype != rgb:
            raise _lib.CrtfxError(_lib.E_UNSUPPORTED, f"only {self._rgb} RGB frames are converted, got {frames.dtype}")
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (h, w, 3) or frames.device != self.device:
            raise ValueError(f"frames must be {self._rgb} [n, {h}, {w}, 3] on {self.device}, got {tuple(frames.shape)} on {frames.device}")
        n = int(frames.shape[0])
        if out is None:
            out = torch.empty((n, self.frame_bytes), dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or tuple(out.shape) != (n, self.frame_bytes) or out.device != self.device:
            raise ValueError(f"out must be uint8 [{n}, {self.frame_bytes}] on {self.device}")
        return self._run(frames, out, n)


class ResizePlan(Handle):
    """A resize stage: out = plan.run(frames[n, src_h, src_w, 3]) -> [n, h, w, 3] of the same dtype (plan(frames) is the same call)."""
    _dtype = "uint8"             # torch dtype of the frames: "uint8" or "float16"
    _refusal = ""                # what a batch of another dtype is told: a format string over {dtype} and {got}

    def __init__(self, device, src_size, dst_size, pix_fmt):
        self._open(device)
        self.src_size = (int(src_size[0]), int(src_size[1]))
        self.dst_size = (int(dst_size[0]), int(dst_size[1]))
        if min(self.src_size + self.dst_size) < 1:
            raise _lib.CrtfxError(_lib.E_INVALID, f"sizes {self.src_size} -> {self.dst_size} must be at least 1 x 1")
        ax = self._axis(self.src_size[1], self.dst_size[1])
        ay = self._axis(self.src_size[0], self.dst_size[0])
        self._create(self.src_size[0], self.src_size[1], self.dst_size[0], self.dst_size[1], int(pix_fmt),
                     tables.ptr(ax[0]), tables.ptr(ax[1]), tables.ptr(ax[2]), ax[2].shape[1],
                     tables.ptr(ay[0]), tables.ptr(ay[1]), tables.ptr(ay[2]), ay[2].shape[1])

    def _axis(self, n_in, n_out):
        """The (min, count, k) tables of one axis: Pillow's BILINEAR ones unless the class says otherwise."""
        return tables.pil_resample_axis(n_in, n_out)

    def run(self, frames, out=None):
        import torch
        (sh, sw), (h, w) = self.src_size, self.dst_size
        dtype = getattr(torch, self._dtype)
        if frames.dtype != dtype:
            raise _lib.CrtfxError(_lib.E_UNSUPPORTED, self._refusal.format(dtype=dtype, got=frames.dtype))
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (sh, sw, 3) or frames.device != self.device:
            raise ValueError(f"frames must be {self._dtype} [n, {sh}, {sw}, 3] on {self.device}, got {tuple(frames.shape)} on {frames.device}")
        n = int(frames.shape[0])
        if out is None:
            out = torch.empty((n, h, w, 3), dtype=dtype, device=self.device)
        if out.dtype != dtype or tuple(out.shape) != (n, h, w, 3) or out.device != self.device:
            raise ValueError(f"out must be {self._dtype} [{n}, {h}, {w}, 3] on {self.device}")
        return self._run(frames, out, n)


def pix_format(dtype, error=ValueError):
    """(torch dtype, C pixel-format number) of a frame stage's `dtype` argument: None (torch.uint8), torch.uint8 or torch.float16."""
    import torch
    dtype = torch.uint8 if dtype is None else dtype
    if dtype not in (torch.uint8, torch.float16):
        raise error(f"dtype must be torch.uint8 or torch.float16, got {dtype!r}")
    return dtype, _lib.PIX_F16 if dtype == torch.float16 else _lib.PIX_U8


class FramePlan(Handle):
    """A frame stage: out = plan.run(frames[n, sh, sw, 3]) -> [ceil(n / frames_in) * frames_out, dh, dw, 3], either side of a dtype of its
    own (plan(frames) is the same call).  A plan says what it takes and gives with `_frames` before it is run."""
    frames_out = 1               # output frames per ...
    frames_in = 1                # ... this many source frames

    def _frames(self, takes, gives=None):
        """(h, w, torch dtype) of one source frame and of one output frame (the same unless given)."""
        self._takes, self._gives = tuple(takes), tuple(gives or takes)

    def _check_frames(self, frames) -> int:
        h, w, dtype = self._takes
        name = str(dtype).replace("torch.", "")
        if frames.dtype != dtype:
            raise _lib.CrtfxError(_lib.E_UNSUPPORTED, f"this plan takes {name} RGB frames, got {frames.dtype}")
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (h, w, 3) or frames.device != self.device:
            raise ValueError(f"frames must be {name} [n, {h}, {w}, 3] on {self.device}, got {tuple(frames.shape)} on {frames.device}")
        return int(frames.shape[0])

    def _check_out(self, n, out):
        import torch
        h, w, dtype = self._gives
        shape = (-(-n // self.frames_in) * self.frames_out, h, w, 3)
        if out is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        if out.dtype != dtype or tuple(out.shape) != shape or out.device != self.device:
            raise ValueError(f"out must be {str(dtype).replace('torch.', '')} {list(shape)} on {self.device}")
        return out

    def run(self, frames, out=None):
        n = self._check_frames(frames)
        return self._run(frames, self._check_out(n, out), n)


def resize_plan(device, src_size, dst_size, filter="bilinear", dtype=None):     # noqa: A002 - the resize plans' keyword
    """The plan that brings RGB frames of `dtype` (torch.uint8 unless given) from one size to another: IngestResize (uint8) or ResizeHalf
    (float16) for "bilinear", Resample under any other filter."""
    import torch
    if filter != "bilinear":
        from .resample import Resample
        return Resample(device, src_size, dst_size, filter=filter, dtype=dtype)
    if dtype == torch.float16:
        from .resize16 import ResizeHalf
        return ResizeHalf(device, src_size, dst_size)
    from .ingest import IngestResize
    return IngestResize(device, src_size, dst_size)
