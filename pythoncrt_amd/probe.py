"""The source probe — what `in_crop`, `deinterlace` / `field_order` and the level keywords of `process_frames` describe, MEASURED on the
device instead of guessed or taken from a separate ffmpeg pass (cropdetect, idet, signalstats).

`Probe` is the plan over include/crtfx_probe.h: RGB frames as a source plan writes them give one record of exact integer statistics each.
`decode` reads records on the host, `ProbeReport` accumulates them and answers `crop()`, `field_order()`, `levels()`, `suggest()` (keywords
of `process_frames`) and `flags()` (flags of pythoncrt_amd.cli).  `probe_frames` runs a whole stream: the frame iterator and the input keywords
of `process_frames`, staged, uploaded and converted the same way.

    report = pythoncrt_amd.probe_frames(iter_yuv420(stream, 720, 480), 720, 480, in_pix_fmt="nv12", max_frames=200)
    n = pythoncrt_amd.process_frames(frames, write, 720, 480, 59.94, in_pix_fmt="nv12", **report.suggest())

    python -m pythoncrt_amd.probe --input tape.nv12 --width 720 --height 480 --in-pix-fmt nv12 --frames 200
    --in-crop-x 0 --in-crop-y 60 --in-crop-width 720 --in-crop-height 360 --deinterlace adaptive --field-order bff

The command prints one line of flags to paste into the render command, or the whole report with `--json`."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable, List, Optional, Tuple

import numpy as np

from . import _lib, formats
from ._stage import FramePlan, pix_format

W_FLAGS, W_MIN, W_MAX, W_SUM, W_CUR, W_EVEN, W_ODD, W_HIST, W_ROWS = 0, 1, 4, 8, 10, 12, 14, 16, 272      # the record's layout (crtfx_probe.h)
LIMIT = 96          # crop(): a row or column is picture where its mean luma exceeds this code in some frame; code 24 of 255, cropdetect's default
# field_order(): E >= RATIO * O is "tff", O >= RATIO * E "bff".  A heuristic: the geometric mean of what progressive scenes show (E / O within
# 1.01 of 1) and what woven ones show (2.2 .. 2.5 where the picture moves; tests/probe_model.py builds such scenes), so that either kind
# keeps a factor of 1.5 to the threshold.
RATIO = 1.52


def words(h: int, w: int) -> int:
    """uint32 words of one record: 272 + h + w rounded up to even (crtfx_probe_words, which needs no plan)."""
    return int(_lib.load().crtfx_probe_words(int(h), int(w)))


class Probe(FramePlan):
    """plan = Probe(device, (h, w), dtype=None); records = plan.run(frames[n, h, w, 3], prev=None) -> uint32 [n, plan.words], the layout of
    include/crtfx_probe.h.  `prev` is the [h, w, 3] frame in front of frames[0], or None: frames[0] then has no previous frame.  It may be a
    view of `frames`; it may not overlap `out`, which is a uint32 [n, plan.words] tensor whose rows start at multiples of 8 bytes.
    plan.push(frames) is run() with the previous frame the plan kept: none at first, then a device copy of the last frame pushed, in a tensor
    the wrapper owns (copied on the current stream behind the kernel); plan.reset() forgets it.  The C plan itself keeps nothing.  `dtype` is
    torch.uint8 (default) or torch.float16.  The work is enqueued on the current stream of `device`; nothing synchronises.  plan.plan() is
    crtfx_probe_last_plan as a dictionary, e.g. {"probe": "k_probe<u8,vec>", "frames": "5"}."""
    _family = "probe"
    _force_option = _lib.PROBE_OPT_FORCE_GENERAL

    def __init__(self, device, size: Tuple[int, int], dtype=None, force_general: bool = False):
        self._kept, self._has_kept = None, False
        self._open(device)
        self.dtype, pix_fmt = pix_format(dtype)
        self.size = (int(size[0]), int(size[1]))
        self._create(self.size[0], self.size[1], pix_fmt)
        self.words = int(self._fn("words")(self.size[0], self.size[1]))
        self._frames(self.size + (self.dtype,))
        if force_general:
            self.force_general = True

    def run(self, frames, prev=None, out=None):
        import torch
        h, w = self.size
        n = self._check_frames(frames)
        if prev is not None and (prev.dtype != self.dtype or tuple(prev.shape) != (h, w, 3) or prev.device != self.device or not prev.is_contiguous()):
            raise ValueError(f"prev must be one contiguous {self.dtype} [{h}, {w}, 3] frame on {self.device}, got {prev.dtype} {tuple(prev.shape)} on {prev.device}")
        if out is None:
            out = torch.empty((n, self.words), dtype=torch.uint32, device=self.device)
        if out.dtype != torch.uint32 or tuple(out.shape) != (n, self.words) or out.device != self.device:
            raise ValueError(f"out must be uint32 [{n}, {self.words}] on {self.device}")
        return self._run(frames, out, n, None if prev is None else prev.data_ptr())

    def __call__(self, frames, out=None):
        return self.run(frames, None, out)

    def push(self, frames, out=None):
        """run() behind the frames pushed before: the previous frame is the last frame of the push before this one (none behind reset() or at
        first).  n = 0 keeps what it had."""
        import torch
        out = self.run(frames, self._kept if self._has_kept else None, out)
        if int(frames.shape[0]):
            if self._kept is None:
                self._kept = torch.empty(self.size + (3,), dtype=self.dtype, device=self.device)
            self._kept.copy_(frames[-1])            # on the current stream, behind the kernel that read the frame kept before
            self._has_kept = True
        return out

    def reset(self) -> None:
        """Forget the kept frame: the next frame pushed has no previous frame (a new stream, a size change, a seek)."""
        self._has_kept = False


# ---- the records on the host ----------------------------------------------------------------------------------------------------------------

@dataclass
class FrameStats:
    """One record, decoded: codes are quarter codes 0..1020 (a uint8 sample u is 4 u), Y the luma of crtfx_probe.h.  The arrays are views of
    the record."""
    had_prev: bool
    rgb_min: Tuple[int, int, int]
    rgb_max: Tuple[int, int, int]
    sum_y: int
    s_cur: int
    s_even: int
    s_odd: int
    hist: np.ndarray        # [256] counts of Y >> 2
    rows: np.ndarray        # [h] sums of Y
    cols: np.ndarray        # [w]


def _host(records) -> np.ndarray:
    a = records.cpu().numpy() if hasattr(records, "cpu") else np.asarray(records)
    if a.dtype != np.uint32 or a.ndim not in (1, 2):
        raise ValueError(f"records are uint32 [n, words] (or one [words]), got {a.dtype} {a.shape}")
    return a.reshape(-1, a.shape[-1])


def decode(records, size: Tuple[int, int]) -> List[FrameStats]:
    """The records (a uint32 [n, words] tensor or array; one [words] record is taken too) of frames of `size` = (h, w), one FrameStats each."""
    h, w = int(size[0]), int(size[1])
    a = _host(records)
    if a.shape[1] != (W_ROWS + h + w + 1) // 2 * 2:
        raise ValueError(f"a record of a {h} x {w} frame holds {(W_ROWS + h + w + 1) // 2 * 2} words, got {a.shape[1]}")

    def u64(r, at):
        return int(r[at]) | int(r[at + 1]) << 32
    return [FrameStats(bool(int(r[W_FLAGS]) & 1), tuple(int(v) for v in r[W_MIN:W_MIN + 3]), tuple(int(v) for v in r[W_MAX:W_MAX + 3]),
                       u64(r, W_SUM), u64(r, W_CUR), u64(r, W_EVEN), u64(r, W_ODD), r[W_HIST:W_HIST + 256], r[W_ROWS:W_ROWS + h],
                       r[W_ROWS + h:W_ROWS + h + w]) for r in a]


class ProbeReport:
    """What the records of a stream of h x w frames say.  report.add(records) takes them batch by batch; everything is kept as host
    integers, so the answers do not depend on how the stream was cut into batches."""

    def __init__(self, size: Tuple[int, int]):
        self.size = (int(size[0]), int(size[1]))
        h, w = self.size
        self.frames = self.pairs = 0                    # records added; those that had a previous frame
        self.s_cur = self.s_even = self.s_odd = 0       # over the pairs
        self.sum_y = 0
        self.rgb_min, self.rgb_max = [1020] * 3, [0] * 3
        self.hist = np.zeros(256, dtype=np.int64)
        self.row_max, self.col_max = np.zeros(h, dtype=np.int64), np.zeros(w, dtype=np.int64)     # the largest sum any frame had

    def add(self, records) -> "ProbeReport":
        for f in decode(records, self.size):
            self.frames += 1
            self.sum_y += f.sum_y
            self.rgb_min = [min(a, b) for a, b in zip(self.rgb_min, f.rgb_min)]
            self.rgb_max = [max(a, b) for a, b in zip(self.rgb_max, f.rgb_max)]
            self.hist += f.hist
            np.maximum(self.row_max, f.rows, out=self.row_max)
            np.maximum(self.col_max, f.cols, out=self.col_max)
            if f.had_prev:
                self.pairs += 1
                self.s_cur, self.s_even, self.s_odd = self.s_cur + f.s_cur, self.s_even + f.s_even, self.s_odd + f.s_odd
        return self

    def crop(self, limit: int = LIMIT, round: int = 2) -> Optional[Tuple[int, int, int, int]]:     # noqa: A002 - cropdetect's word
        """(y, x, h, w) of the picture area, or None.  A row belongs to the picture if its sum of Y exceeds limit * w in some frame, a column
        if it exceeds limit * h; the window spans the first to the last such row and column and is shrunk inward to multiples of `round`
        (2: what a 4:2:0 source can be cut at).  None where the window is the whole frame, and where no row or column qualifies."""
        h, w = self.size
        round = max(1, int(round))
        ys, xs = np.flatnonzero(self.row_max > int(limit) * w), np.flatnonzero(self.col_max > int(limit) * h)
        if not ys.size or not xs.size:
            return None
        y0, y1, x0, x1 = (-(-int(ys[0]) // round) * round, (int(ys[-1]) + 1) // round * round,
                          -(-int(xs[0]) // round) * round, (int(xs[-1]) + 1) // round * round)
        if y1 <= y0 or x1 <= x0 or (y0, x0, y1, x1) == (0, 0, h, w):
            return None
        return y0, x0, y1 - y0, x1 - x0

    def field_order(self, ratio: float = RATIO) -> Optional[str]:
        """"tff" where S_even >= ratio * S_odd over the frames that had a previous frame, "bff" where S_odd >= ratio * S_even, else
        "progressive"; None without such a frame or where both sums are 0 (a still picture says nothing)."""
        e, o = self.s_even, self.s_odd
        if not self.pairs or (e == 0 and o == 0):
            return None
        return "tff" if e >= ratio * o else "bff" if o >= ratio * e else "progressive"

    def levels(self) -> dict:
        """On the 0..255 scale: per-channel min / max, luma min / max / mean, the 0.1 % and 99.9 % points of the summed luma histogram (the
        lowest bin at which at least that share of the pixels lies at or below it) and the share of pixels in bins 0 and 255."""
        total = int(self.hist.sum())
        if not total:
            return {}
        filled = np.flatnonzero(self.hist)
        cum = np.cumsum(self.hist)
        point = lambda share: int(np.searchsorted(cum, share * total, side="left"))      # noqa: E731
        return {"r_min": self.rgb_min[0] / 4, "g_min": self.rgb_min[1] / 4, "b_min": self.rgb_min[2] / 4,
                "r_max": self.rgb_max[0] / 4, "g_max": self.rgb_max[1] / 4, "b_max": self.rgb_max[2] / 4,
                "luma_min": int(filled[0]), "luma_max": int(filled[-1]), "luma_mean": self.sum_y / (4.0 * total),
                "luma_low": point(0.001), "luma_high": point(0.999),
                "black_share": int(self.hist[0]) / total, "white_share": int(self.hist[255]) / total}

    def suggest(self) -> dict:
        """Keywords of `process_frames`: `in_crop` where there are bars; `deinterlace="adaptive"` with the `field_order` where the frames are
        woven fields."""
        kw = {}
        crop, order = self.crop(), self.field_order()
        if crop is not None:
            kw["in_crop"] = crop
        if order in ("tff", "bff"):
            kw.update(deinterlace="adaptive", field_order=order)
        return kw

    def flags(self) -> List[str]:
        """suggest() as flags of pythoncrt_amd.cli."""
        kw, out = self.suggest(), []
        if "in_crop" in kw:
            y, x, ch, cw = kw["in_crop"]
            out += ["--in-crop-x", str(x), "--in-crop-y", str(y), "--in-crop-width", str(cw), "--in-crop-height", str(ch)]
        if "deinterlace" in kw:
            out += ["--deinterlace", kw["deinterlace"], "--field-order", kw["field_order"]]
        return out

    def as_dict(self) -> dict:
        """The report as plain values (json.dumps takes it)."""
        crop = self.crop()
        return {"size": list(self.size), "frames": self.frames, "pairs": self.pairs, "crop": None if crop is None else list(crop),
                "field_order": self.field_order(), "s_cur": self.s_cur, "s_even": self.s_even, "s_odd": self.s_odd, "levels": self.levels(),
                "suggest": {k: list(v) if isinstance(v, tuple) else v for k, v in self.suggest().items()}, "flags": self.flags()}


# ---- a whole stream -------------------------------------------------------------------------------------------------------------------------

def _refuse_input(out_w, out_h, in_pix_fmt, in_matrix, in_range, in_size, in_chroma, surface="keywords", in_chroma_rows="progressive"):
    """The input keywords against options.RULES in `process_frames`' wording (or, for "flags", the CLI's): a Raw that holds its defaults for everything else — but for
    `out_pix_fmt`, which takes a 10-bit input's own name: the rule about one 10-bit end is about a delivery, and the probe has none."""
    from .options import Raw, refuse
    out_fmt = in_pix_fmt if in_pix_fmt in formats.FORMATS and formats.bits(in_pix_fmt) == 10 else "rgb24"
    v = Raw(render_hw=(int(out_h), int(out_w)), resize_on="device", out_pix_fmt=out_fmt, out_matrix="bt601", out_range="tv",
            in_pix_fmt=in_pix_fmt, in_matrix=in_matrix, in_range=in_range, in_size=in_size, in_chroma=in_chroma, out_chroma="center",
            deliver_size=None, in_filter="bilinear", deliver_filter="bilinear", in_crop=None, deliver_fit="stretch", deliver_pad_color=(0, 0, 0),
            chain_pix="auto", dither="none", deinterlace="off", field_order="tff", deinterlace_fields="first", in_lut=None, deliver_lut=None,
            deliver_interlace="off", deliver_lowpass="none", in_signal="rgb", signal_chroma="sharp", signal_crawl=True, in_chroma_rows=in_chroma_rows)
    refuse(v, surface)
    return v.src_hw


def probe_frames(frame_iter: Iterable[np.ndarray], out_w: int, out_h: int, *, in_pix_fmt: str = "rgb24", in_matrix: str = "bt601",
                 in_range: str = "tv", in_size: Optional[Tuple[int, int]] = None, in_chroma: str = "replicate",
                 max_frames: Optional[int] = None, batch: int = 16, device=None, in_chroma_rows: str = "progressive") -> ProbeReport:
    """Probe the frames of `frame_iter` — what `process_frames` would be given, with its input keywords — and return the ProbeReport.
    A packed `in_pix_fmt` has frames of `in_size` (default: out_h x out_w) as 1-D arrays of formats.frame_bytes bytes; they are staged in
    pinned memory, uploaded and converted to RGB by formats.source_plan as `process_frames` does, 10-bit formats to half frames.  "rgb24"
    frames are H x W x 3 arrays and are probed as they are, at their own size, which must be one size: a second size raises ValueError.
    `Probe.push` runs batch after batch of `batch` frames, so every frame but the first has a previous frame; the records are downloaded and
    added to the report.  `max_frames` stops early.  `in_chroma_rows="interlaced"` reads a 4:2:0 input as an interlaced encoder wrote it,
    every luma row taking chroma from rows of its own field (UnpackField420, as under `process_frames`): the field-order measure then sees
    the asymmetry of coloured motion undiminished.  The keywords are refused as `process_frames` refuses them (options.RULES, the same
    messages), before a device is touched."""
    import torch
    src_hw = _refuse_input(out_w, out_h, in_pix_fmt, in_matrix, in_range, in_size, in_chroma, in_chroma_rows=in_chroma_rows)
    if max_frames is not None and int(max_frames) < 0:
        raise ValueError(f"max_frames must be None or >= 0, got {max_frames!r}")
    if not torch.cuda.is_available():
        raise RuntimeError("no ROCm device visible; pythoncrt_amd has no CPU fallback")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    B = max(1, int(batch))
    packed = in_pix_fmt != "rgb24"
    deep = formats.bits(in_pix_fmt) == 10
    state = {}                                       # built at the first frame: an rgb24 stream brings its size

    def setup(hw):
        shape = (formats.frame_bytes(hw[0], hw[1], in_pix_fmt),) if packed else hw + (3,)
        state.update(hw=hw, shape=shape, report=ProbeReport(hw), pin=torch.empty((B,) + shape, dtype=torch.uint8).pin_memory(),
                     dev=torch.empty((B,) + shape, dtype=torch.uint8, device=dev),
                     source=formats.source_plan(dev, hw, in_pix_fmt, in_matrix, in_range, in_chroma,
                                                *(() if in_chroma_rows == "progressive" else (in_chroma_rows,))),
                     probe=Probe(dev, hw, dtype=torch.float16 if deep else torch.uint8))
        state["np"] = state["pin"].numpy()

    def flush(n):
        state["dev"][:n].copy_(state["pin"][:n], non_blocking=True)
        rgb = state["dev"][:n] if state["source"] is None else state["source"].run(state["dev"][:n])
        state["report"].add(state["probe"].push(rgb).cpu())      # the download waits for the kernels: the pinned slot is free again

    n = taken = 0
    for frame in frame_iter:
        if max_frames is not None and taken >= int(max_frames):
            break
        a = np.asarray(frame)
        if packed:
            a = a.reshape(-1)
            if deep and a.dtype.itemsize in (2, 4):
                a = np.ascontiguousarray(a).view(np.uint8)
            if not state:
                setup(src_hw)
            if a.size != state["shape"][0]:
                raise ValueError(f"a {in_pix_fmt} frame of {src_hw[0]} x {src_hw[1]} holds {state['shape'][0]} bytes, got an item of {a.size}")
        else:
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"frames must be H x W x 3 RGB arrays, got {a.shape}")
            if not state:
                setup((int(a.shape[0]), int(a.shape[1])))
            if tuple(a.shape[:2]) != state["hw"]:
                raise ValueError(f"rgb24 frames of more than one size: {a.shape[0]} x {a.shape[1]} behind {state['hw'][0]} x {state['hw'][1]} "
                                 "(probe each size on its own)")
        np.copyto(state["np"][n], a, casting="unsafe")
        n, taken = n + 1, taken + 1
        if n == B:
            flush(n)
            n = 0
    if n:
        flush(n)
    if not state:
        return ProbeReport(src_hw if src_hw is not None else (int(out_h), int(out_w)))
    state["probe"].close()
    return state["report"]


# ---- python -m pythoncrt_amd.probe ----------------------------------------------------------------------------------------------------------

def build_parser():
    import argparse
    from . import cli
    p = argparse.ArgumentParser(prog="python -m pythoncrt_amd.probe", description="Measure the letterbox, the field order and the levels of a raw "
                                "video file on the GPU and print the flags of pythoncrt_amd.cli that describe them.")
    p.add_argument("--input", type=str, required=True, metavar="FILE|-", help="raw frames of --in-pix-fmt at --width x --height; - = standard input")
    p.add_argument("--width", type=int, required=True)
    p.add_argument("--height", type=int, required=True)
    full = cli.add_input_flags(argparse.ArgumentParser(add_help=False))      # cli's own choices and help of the five flags, not restated
    for action in full._actions:
        if action.option_strings and action.option_strings[0] in ("--in-pix-fmt", "--in-matrix", "--in-range", "--in-chroma", "--in-chroma-rows"):
            p.add_argument(*action.option_strings, type=action.type, default=action.default, choices=action.choices, help=action.help)
    p.add_argument("--frames", type=int, default=0, metavar="N", help="probe the first N frames only; 0 (default) = the whole input")
    p.add_argument("--json", action="store_true", help="print the whole report as one JSON object instead of the line of flags")
    return p


def main(argv=None) -> int:
    import json
    import sys
    from .options import OptionError
    from .render import _iter_frames
    a = build_parser().parse_args(argv)
    if a.width <= 0 or a.height <= 0:
        raise SystemExit("raw input needs --width and --height")
    if a.frames < 0:
        raise SystemExit(f"--frames {a.frames}: pass a count, or 0 for the whole input")
    try:
        _refuse_input(a.width, a.height, a.in_pix_fmt, a.in_matrix, a.in_range, None, a.in_chroma, "flags", a.in_chroma_rows)
    except OptionError as e:
        raise SystemExit(str(e)) from e
    fin = sys.stdin.buffer if a.input == "-" else open(a.input, "rb")
    try:
        items = _iter_frames(fin, formats.frame_bytes(a.height, a.width, a.in_pix_fmt))
        if a.in_pix_fmt == "rgb24":
            items = (f.reshape(a.height, a.width, 3) for f in items)
        report = probe_frames(items, a.width, a.height, in_pix_fmt=a.in_pix_fmt, in_matrix=a.in_matrix, in_range=a.in_range,
                              in_chroma=a.in_chroma, max_frames=a.frames or None, in_chroma_rows=a.in_chroma_rows)
    finally:
        if fin is not sys.stdin.buffer:
            fin.close()
    print(json.dumps(report.as_dict()) if a.json else " ".join(report.flags()))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
