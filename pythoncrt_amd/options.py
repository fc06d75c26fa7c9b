"""`ChainOptions` — the validated description of what stands around the effect chain — and RULES, the one ordered table of what
`process_frames` (keywords) and the CLI (flags) refuse.  An entry is a predicate over the raw values and the message it raises on each
surface, side by side; an entry with one message exists on that surface only (`resize_on="host"`, `in_size`, the membership checks argparse
makes for the CLI, the parsers of the API's loose values).  What both callers derive from the options, the two ends included, is a property
or method of the spec.  No torch here: every refusal comes before a device, and on the command line before torch is imported."""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace
from typing import Callable, NamedTuple, Optional, Tuple

from . import field420, formats, render, sited, tables
from .adeint import METHOD as ADAPTIVE
from .cube import Cube, as_cube
from .deint import FIELDS, METHODS as SPATIAL, ORDERS
from .depth import DITHERS
from .interlace import LOWPASS, ORDERS as WEAVE_ORDERS
from .pal import DECODERS, PHASES
from .signal import CHROMAS, SIGNALS


class OptionError(ValueError):
    """A combination of options that RULES refuses; `rule` names the entry."""

    def __init__(self, text: str, rule: str):
        super().__init__(text)
        self.rule = rule


class Raw(SimpleNamespace):
    """The raw values of either surface, under `process_frames`' keyword names, and `render_hw`; the parsers among RULES replace a loose
    value (in_crop, deliver_pad_color, deliver_size, in_lut, deliver_lut) by its canonical one.  Below: what predicates and messages read."""
    deep_in = property(lambda v: formats.bits(v.in_pix_fmt) == 10)
    deep_out = property(lambda v: formats.bits(v.out_pix_fmt) == 10)
    in_size_given = property(lambda v: tuple(v.in_size))
    crop_bounds = property(lambda v: None if v.in_pix_fmt == "rgb24" else v.src_hw)
    rows = property(lambda v: (v.deliver_size or v.render_hw)[0])      # of a delivered frame; None: the CLI's --height, not checked yet
    crawl = property(lambda v: "on" if v.signal_crawl else "off")
    in_chroma_rows = "progressive"      # unless the surface says otherwise
    out_chroma_rows = "progressive"     # likewise
    signal_standard = "ntsc"            # likewise: the three values of PAL_RULES
    pal_decoder = "delay"
    signal_phase = 0

    @property
    def src_rows(v):
        """The rows of a source frame where the options fix them; None for rgb24 frames and for a --height not checked yet."""
        size = v.in_size if v.in_size is not None else v.render_hw if v.in_pix_fmt != "rgb24" else None
        return None if size is None or size[0] is None else int(size[0])

    @property
    def src_hw(v):
        """The source size where the options fix it: `in_size`, or the render size for a packed format; None for rgb24 frames, which bring their own."""
        if v.in_size is not None:
            return int(v.in_size[0]), int(v.in_size[1])
        return v.render_hw if v.in_pix_fmt != "rgb24" else None


class Rule(NamedTuple):
    name: str
    broken: Callable                    # Raw -> true where refused; a parser stores the canonical value and raises its own message
    keywords: Optional[str] = None      # the ValueError text of process_frames, formatted with v = the Raw; None: no rule of the keyword API
    flags: Optional[str] = None         # the exit text of the CLI; None: no rule of the CLI (argparse, or a parser of cli.py, has it)
    early: bool = False                 # flags: checked in front of the sharded CLI's branch, which has refusals of its own for the rest


def _member(name, allowed, text=None, kind=object, tail=""):
    """The keyword API's membership check of `name` (argparse's `choices` on the command line)."""
    return Rule(name, lambda v: not isinstance(getattr(v, name), kind) or getattr(v, name) not in allowed,
                (text or f"{name} must be one of {', '.join(allowed)}") + f", got {{v.{name}!r}}" + tail)


def _on_host(name, on, why):
    return Rule(name, lambda v: v.resize_on == "host" and on(v), "resize_on='host' cannot be combined with " + why)


def _parsed(name, parse):
    def step(v):
        setattr(v, name, parse(v))
    return Rule(name, step, "")


def _cube(name):
    return _parsed(name, lambda v: None if getattr(v, name) is None else as_cube(getattr(v, name), name))


METHODS = SPATIAL + (ADAPTIVE,)
PIX_FMTS = ("{} must be 'rgb24', 'yuv420p' or 'nv12', 'yuv422p', 'yuyv422' or 'uyvy422' (or, with a 10-bit {}, 'yuv420p10le' or 'p010le', "
            "'yuv444p10le', 'gbrp10le' or 'x2rgb10le')")
SITED, NO_RESIZE = f"({', '.join(sited.LAYOUTS)})", "a 10-bit input cannot be resized (IngestResize has no half path)"
NO_DELIVERY_K, NO_DELIVERY_F = "without a deliver_size that differs from the render size", "without --deliver-width / --deliver-height other than the render size"

RULES = (
    _member("resize_on", ("device", "host"), "resize_on must be 'device' or 'host'"),
    _member("out_pix_fmt", formats.PIX_FMTS, PIX_FMTS.format("out_pix_fmt", "input")),
    _member("in_pix_fmt", formats.PIX_FMTS, PIX_FMTS.format("in_pix_fmt", "output")),
    _member("in_chroma", ("replicate", "left", "center"), "in_chroma must be 'replicate', 'left' or 'center'"),
    Rule("in_chroma_format", lambda v: v.in_chroma != "replicate" and v.in_pix_fmt not in sited.LAYOUTS,
         "in_chroma={v.in_chroma!r} with in_pix_fmt={v.in_pix_fmt!r}: only a 4:2:0 or 4:2:2 input has sub-sampled chroma to interpolate " + SITED,
         "--in-chroma {v.in_chroma} with --in-pix-fmt {v.in_pix_fmt}: only a 4:2:0 or 4:2:2 input has sub-sampled chroma to interpolate " + SITED, early=True),
    _member("out_chroma", ("center", "left"), "out_chroma must be 'center' or 'left'"),
    Rule("out_chroma_format", lambda v: v.out_chroma != "center" and v.out_pix_fmt not in sited.LAYOUTS,
         "out_chroma={v.out_chroma!r} with out_pix_fmt={v.out_pix_fmt!r}: only a 4:2:0 or 4:2:2 output has chroma to down-sample " + SITED,
         "--out-chroma {v.out_chroma} with --out-pix-fmt {v.out_pix_fmt}: only a 4:2:0 or 4:2:2 output has chroma to down-sample " + SITED, early=True),
    _parsed("in_crop", lambda v: render.parse_in_crop(v.in_crop, v.crop_bounds)),
    _on_host("in_crop_host", lambda v: v.in_crop is not None, "in_crop={v.in_crop}: the window is cut on the device"),
    _member("deliver_fit", render.DELIVER_FITS),
    _parsed("deliver_pad_color", lambda v: render.parse_pad_color(v.deliver_pad_color)),
    _member("chain_pix", render.CHAIN_PIX, tail=" (dither={v.dither!r})"),
    _member("dither", DITHERS, tail=" (chain_pix={v.chain_pix!r})"),
    _member("deinterlace", ("off",) + METHODS, f"deinterlace must be 'off' or one of {', '.join(METHODS)}"),
    _member("field_order", ORDERS),
    _member("deinterlace_fields", FIELDS),
    Rule("deinterlace_off", lambda v: v.deinterlace == "off" and (v.field_order != "tff" or v.deinterlace_fields != "first"),
         "field_order={v.field_order!r} / deinterlace_fields={v.deinterlace_fields!r} with deinterlace='off': there is nothing to deinterlace",
         "--field-order {v.field_order} / --deinterlace-fields {v.deinterlace_fields} without --deinterlace linear | edge | adaptive: there is nothing to deinterlace",
         early=True),
    _on_host("deinterlace_host", lambda v: v.deinterlace != "off",
             "deinterlace={v.deinterlace!r}: the fields are separated on the device, in front of the resize"),
    Rule("deinterlace_rows", lambda v: v.deinterlace != "off" and v.src_hw is not None and v.src_hw[0] < 2,
         "deinterlace={v.deinterlace!r}: a source frame of {v.src_hw[0]} row(s) has no two fields",
         "--deinterlace {v.deinterlace} with --height {v.render_hw[0]}: a frame of one row has no two fields"),
    Rule("dither_unused", lambda v: v.dither != "none" and (v.chain_pix != "half" or v.deep_out),
         "dither={v.dither!r} with chain_pix={v.chain_pix!r} and out_pix_fmt={v.out_pix_fmt!r}: only half frames narrowed to an 8-bit "
         "delivery are dithered (chain_pix='half' and an 8-bit or rgb24 out_pix_fmt)",
         "--dither {v.dither} with --chain-pix {v.chain_pix} and --out-pix-fmt {v.out_pix_fmt}: only half frames narrowed to an 8-bit output "
         "are dithered; pass --chain-pix half and an 8-bit or rgb24 --out-pix-fmt", early=True),
    Rule("one_deep_end", lambda v: v.chain_pix != "half" and v.deep_in != v.deep_out,                       # under "auto": both ends or neither
         "in_pix_fmt={v.in_pix_fmt!r} with out_pix_fmt={v.out_pix_fmt!r}: a 10-bit format on one end only — the chain between "
         "them runs on half pixels or on uint8 ones, and the 8-bit stages have no half path (the 10-bit ones no uint8 path)",
         "--in-pix-fmt {v.in_pix_fmt} with --out-pix-fmt {v.out_pix_fmt}: a 10-bit format on one end only; the chain between them runs on half "
         "pixels or on uint8 ones — pass yuv420p10le / p010le (or yuv444p10le / gbrp10le / x2rgb10le) on both ends or on neither"),
    Rule("deep_crop", lambda v: v.deep_in and v.in_crop is not None and v.in_crop[2:] != v.render_hw,
         "in_crop={v.in_crop} leaves a {v.in_crop[2]} x {v.in_crop[3]} window that differs from the output size {v.render_hw}: " + NO_RESIZE,
         "--in-crop-width {v.in_crop[3]} --in-crop-height {v.in_crop[2]} differs from --width {v.render_hw[1]} x --height {v.render_hw[0]}: " + NO_RESIZE),
    Rule("deep_in_size", lambda v: v.deep_in and v.in_crop is None and v.in_size is not None and v.src_hw != v.render_hw,
         "in_size={v.in_size_given} differs from the output size {v.render_hw}: " + NO_RESIZE),
    _on_host("packed_host", lambda v: v.in_pix_fmt != "rgb24", "in_pix_fmt={v.in_pix_fmt!r}: there is no host RGB frame to hand to Pillow"),
    _parsed("deliver_size", lambda v: render.parse_deliver_size(v.deliver_size, *v.render_hw)),
    _member("in_filter", tables.RESAMPLE_FILTERS),
    _member("deliver_filter", tables.RESAMPLE_FILTERS),
    Rule("deliver_filter_unused", lambda v: v.deliver_filter != "bilinear" and v.deliver_size is None,
         "deliver_filter={v.deliver_filter!r} " + NO_DELIVERY_K + ": there is no delivery resize to filter",
         "--deliver-filter {v.deliver_filter} " + NO_DELIVERY_F + ": there is no delivery resize to filter"),
    Rule("deliver_fit_unused", lambda v: v.deliver_fit != "stretch" and v.deliver_size is None,
         "deliver_fit={v.deliver_fit!r} " + NO_DELIVERY_K + ": there is nothing to fit", "--deliver-fit {v.deliver_fit} " + NO_DELIVERY_F + ": there is nothing to fit"),
    _member("deliver_interlace", ("off",) + WEAVE_ORDERS, f"deliver_interlace must be 'off' or one of {', '.join(WEAVE_ORDERS)}"),
    _member("deliver_lowpass", LOWPASS),
    Rule("deliver_lowpass_unused", lambda v: v.deliver_interlace == "off" and v.deliver_lowpass != "none",
         "deliver_lowpass={v.deliver_lowpass!r} with deliver_interlace='off': there is nothing to filter",
         "--deliver-lowpass {v.deliver_lowpass} without --deliver-interlace tff | bff: there is nothing to filter", early=True),
    Rule("weave_rows", lambda v: v.deliver_interlace != "off" and v.rows is not None and v.rows < 2,
         "deliver_interlace={v.deliver_interlace!r}: a delivered frame of {v.rows} row(s) has no two fields",
         "--deliver-interlace {v.deliver_interlace} with a delivery height of {v.rows}: a frame of one row has no two fields", early=True),
    _member("in_signal", ("rgb",) + SIGNALS, f"in_signal must be 'rgb' or one of {', '.join(SIGNALS)}", kind=str),
    _member("signal_chroma", CHROMAS, kind=str),
    _member("signal_crawl", (True, False), "signal_crawl must be True or False", kind=bool),
    Rule("signal_off", lambda v: v.in_signal == "rgb" and (v.signal_chroma != "sharp" or not v.signal_crawl),
         "signal_chroma={v.signal_chroma!r} / signal_crawl={v.signal_crawl!r} with in_signal='rgb': there is no signal to decode",
         "--signal-chroma {v.signal_chroma} / --signal-crawl {v.crawl} without --in-signal composite | svideo: there is no signal to decode", early=True),
    _on_host("signal_host", lambda v: v.in_signal != "rgb",
             "in_signal={v.in_signal!r}: the signal is formed on the device, at the source's size, in front of the device's resize"),
    _on_host("in_lut_host", lambda v: v.in_lut is not None, "in_lut: the cube is applied on the device, behind the device's resize"),
    _cube("in_lut"),
    _cube("deliver_lut"),
)


CHROMA_ROWS = ("progressive", "interlaced")
FIELD420 = f"({', '.join(field420.LAYOUTS)})"

# What in_chroma_rows adds, walked behind RULES: a table of its own, every entry in front of the sharded CLI's branch.
FIELD_RULES = (
    Rule("in_chroma_rows", lambda v: not isinstance(v.in_chroma_rows, str) or v.in_chroma_rows not in CHROMA_ROWS,
         "in_chroma_rows must be 'progressive' or 'interlaced', got {v.in_chroma_rows!r}", early=True),
    Rule("in_chroma_rows_format", lambda v: v.in_chroma_rows == "interlaced" and v.in_pix_fmt not in field420.LAYOUTS,
         "in_chroma_rows='interlaced' with in_pix_fmt={v.in_pix_fmt!r}: only a 4:2:0 input has chroma rows that two fields share " + FIELD420,
         "--in-chroma-rows interlaced with --in-pix-fmt {v.in_pix_fmt}: only a 4:2:0 input has chroma rows that two fields share " + FIELD420, early=True),
    Rule("in_chroma_rows_height", lambda v: v.in_chroma_rows == "interlaced" and v.src_rows is not None and (v.src_rows % 2 == 1 or v.src_rows < field420.MIN_ROWS),
         "in_chroma_rows='interlaced': a source frame of {v.src_rows} row(s) has no two fields of whole chroma rows (an even height of at least 4)",
         "--in-chroma-rows interlaced with --height {v.src_rows}: a frame of {v.src_rows} row(s) has no two fields of whole chroma rows "
         "(an even height of at least 4)", early=True),
)


# What out_chroma_rows adds, walked behind FIELD_RULES: again a table of its own, every entry in front of the sharded CLI's branch.  It does
# not ask for deliver_interlace: a woven source passed through undeinterlaced is interlaced too.
OUT_FIELD_RULES = (
    Rule("out_chroma_rows", lambda v: not isinstance(v.out_chroma_rows, str) or v.out_chroma_rows not in CHROMA_ROWS,
         "out_chroma_rows must be 'progressive' or 'interlaced', got {v.out_chroma_rows!r}", early=True),
    Rule("out_chroma_rows_format", lambda v: v.out_chroma_rows == "interlaced" and v.out_pix_fmt not in field420.LAYOUTS,
         "out_chroma_rows='interlaced' with out_pix_fmt={v.out_pix_fmt!r}: only a 4:2:0 output has chroma rows that two fields share " + FIELD420,
         "--out-chroma-rows interlaced with --out-pix-fmt {v.out_pix_fmt}: only a 4:2:0 output has chroma rows that two fields share " + FIELD420, early=True),
    Rule("out_chroma_rows_height", lambda v: v.out_chroma_rows == "interlaced" and v.rows is not None and (v.rows % field420.EGRESS_ROWS != 0 or v.rows < field420.EGRESS_ROWS),
         "out_chroma_rows='interlaced': a delivered frame of {v.rows} row(s) has no two fields with whole pairs of luma rows under their chroma rows "
         "(a height that is a multiple of 4)",
         "--out-chroma-rows interlaced with a delivery height of {v.rows}: a frame of {v.rows} row(s) has no two fields with whole pairs of luma rows "
         "under their chroma rows (a height that is a multiple of 4)", early=True),
)


STANDARDS = ("ntsc", "pal")

# What signal_standard adds, walked behind OUT_FIELD_RULES: a table of its own once more, every entry in front of the sharded CLI's branch.
# "ntsc" is the Signal of in_signal as it was; "pal" puts a PalSignal in its place, and only that one has a decoder and a phase knob.
PAL_RULES = (
    Rule("signal_standard", lambda v: not isinstance(v.signal_standard, str) or v.signal_standard not in STANDARDS,
         "signal_standard must be 'ntsc' or 'pal', got {v.signal_standard!r}", early=True),
    Rule("pal_decoder", lambda v: not isinstance(v.pal_decoder, str) or v.pal_decoder not in DECODERS,
         "pal_decoder must be 'delay' or 'simple', got {v.pal_decoder!r}", early=True),
    Rule("signal_phase", lambda v: isinstance(v.signal_phase, bool) or not isinstance(v.signal_phase, int) or not PHASES[0] <= v.signal_phase <= PHASES[1],
         "signal_phase must be an integer number of degrees in -180..180, got {v.signal_phase!r}",
         "--signal-phase {v.signal_phase}: the decoder's phase error is a number of degrees in -180..180", early=True),
    Rule("pal_off", lambda v: v.signal_standard == "ntsc" and (v.pal_decoder != "delay" or v.signal_phase != 0),
         "pal_decoder={v.pal_decoder!r} / signal_phase={v.signal_phase!r} with signal_standard='ntsc': only the PAL decoder has a delay line and a phase knob",
         "--pal-decoder {v.pal_decoder} / --signal-phase {v.signal_phase} without --signal-standard pal: only the PAL decoder has a delay line and "
         "a phase knob", early=True),
    Rule("pal_signal", lambda v: v.signal_standard == "pal" and v.in_signal == "rgb",
         "signal_standard='pal' with in_signal='rgb': there is no signal to decode",
         "--signal-standard pal without --in-signal composite | svideo: there is no signal to decode", early=True),
)


def refuse(v: Raw, surface: str, early: Optional[bool] = None) -> None:
    """Walk RULES, then FIELD_RULES, then OUT_FIELD_RULES, then PAL_RULES, over `v` for `surface` ("keywords" or "flags") and raise OptionError with the first message that
    applies.  `early`: only the entries in front of (True) or behind (False) the CLI's sharded branch."""
    for rule in RULES + FIELD_RULES + OUT_FIELD_RULES + PAL_RULES:
        text = getattr(rule, surface)
        if text is None or early not in (None, rule.early):
            continue
        try:
            if not rule.broken(v):
                continue
        except ValueError as e:         # a parser's own message
            raise OptionError(str(e), rule.name) from None
        raise OptionError(text.format(v=v), rule.name)


@dataclass(frozen=True)
class ChainOptions:
    """Canonical values only: what `refuse` has let through, with every "off" spelt None."""
    render_hw: Tuple[int, int]
    in_pix_fmt: str = "rgb24"
    in_matrix: str = "bt601"
    in_range: str = "tv"
    in_chroma: str = "replicate"
    in_size: Optional[Tuple[int, int]] = None                   # None: the render size
    in_filter: str = "bilinear"
    crop: Optional[Tuple[int, int, int, int]] = None            # (y, x, h, w)
    deinterlace: Optional[Tuple[str, str, str]] = None          # (method, order, fields)
    signal: Optional[Tuple[str, str, bool]] = None              # (signal, chroma, crawl)
    in_cube: Optional[Cube] = None
    chain_pix: str = "auto"
    dither: str = "none"
    out_pix_fmt: str = "rgb24"
    out_matrix: str = "bt601"
    out_range: str = "tv"
    out_chroma: str = "center"
    deliver: Optional[Tuple[int, int]] = None                   # (dh, dw), differing from the render size
    deliver_filter: str = "bilinear"
    deliver_fit: str = "stretch"
    pad_color: Tuple[int, int, int] = (0, 0, 0)
    deliver_cube: Optional[Cube] = None
    weave: Optional[Tuple[str, str]] = None                     # (order, lowpass)
    resize_on: str = "device"
    in_chroma_rows = "progressive"      # a constant here and a field of FieldChainOptions: see there
    out_chroma_rows = "progressive"     # likewise
    signal_standard = "ntsc"            # constants here and fields of PalChainOptions / PalFieldChainOptions
    pal_decoder = "delay"
    signal_phase = 0

    @classmethod
    def build(cls, v: Raw, surface: Optional[str] = None) -> "ChainOptions":
        """The spec of raw values; with a surface they go through `refuse` first (OptionError), without one the caller has done that."""
        if surface is not None:
            refuse(v, surface)
        if cls is ChainOptions:
            fields, pal = v.in_chroma_rows != "progressive" or v.out_chroma_rows != "progressive", v.signal_standard == "pal"
            if fields or pal:
                return {(True, False): FieldChainOptions, (False, True): PalChainOptions, (True, True): PalFieldChainOptions}[fields, pal].build(v)
        rows = {"in_chroma_rows": v.in_chroma_rows, "out_chroma_rows": v.out_chroma_rows} if issubclass(cls, FieldChainOptions) else {}
        if "signal_standard" in cls.__dataclass_fields__:
            rows.update(signal_standard=v.signal_standard, pal_decoder=v.pal_decoder, signal_phase=v.signal_phase)
        return cls(**rows, render_hw=v.render_hw, in_pix_fmt=v.in_pix_fmt, in_matrix=v.in_matrix, in_range=v.in_range, in_chroma=v.in_chroma,
                   in_size=None if v.in_size is None else v.src_hw, in_filter=v.in_filter, crop=v.in_crop,
                   deinterlace=None if v.deinterlace == "off" else (v.deinterlace, v.field_order, v.deinterlace_fields),
                   signal=None if v.in_signal == "rgb" else (v.in_signal, v.signal_chroma, v.signal_crawl), in_cube=v.in_lut,
                   chain_pix=v.chain_pix, dither=v.dither, out_pix_fmt=v.out_pix_fmt, out_matrix=v.out_matrix, out_range=v.out_range,
                   out_chroma=v.out_chroma, deliver=v.deliver_size, deliver_filter=v.deliver_filter, deliver_fit=v.deliver_fit,
                   pad_color=v.deliver_pad_color, deliver_cube=v.deliver_lut,
                   weave=None if v.deliver_interlace == "off" else (v.deliver_interlace, v.deliver_lowpass), resize_on=v.resize_on)

    def _depth(self):
        from .ends import depth_stages
        return depth_stages(self.in_pix_fmt, self.out_pix_fmt, self.chain_pix, self.dither)

    half = property(lambda self: self._depth()[0])          # the chain runs on half pixels: 10-bit formats on both ends, or chain_pix="half"
    widen = property(lambda self: self._depth()[1])         # the source's uint8 stages in front of a half chain end in a Widen
    narrow = property(lambda self: self._depth()[2])        # the dither of the Narrow in front of an 8-bit delivery behind a half chain, or None
    pal = property(lambda self: (self.pal_decoder, self.signal_phase) if self.signal_standard == "pal" else None)   # the PalSignal's own two values
    ratio = property(lambda self: 2 if self.deinterlace is not None and self.deinterlace[2] == "both" else 1)      # frames the chain runs per source frame

    def batch(self, B: int) -> Tuple[int, int]:
        """(the chain's batch, source frames per batch) for a requested batch: even and at least 2 where the chain's frames come or go in
        pairs — both fields of B // 2 source frames, whole pairs for the Interlace."""
        B = max(1, int(B))
        if self.ratio == 2 or self.weave is not None:
            B = max(2, B - B % 2)
        return B, B // self.ratio

    @property
    def direct(self) -> bool:
        """Is an rgb24 frame at render size uploaded straight into the chain's input?  Any stage in front of the chain but the resize of an
        off-size frame says no: such a frame goes through a source end, whose only stage may be that one."""
        return (self.in_pix_fmt == "rgb24" and self.crop is None and not self.widen and self.deinterlace is None and self.in_cube is None
                and self.signal is None)

    def source_end(self, device, src_hw, pix):
        """The SourceEnd of frames of `src_hw` in front of a chain of `pix`."""
        from .ends import SourceEnd
        return SourceEnd(device, self.render_hw, self.in_pix_fmt, self.in_matrix, self.in_range, self.in_chroma, src_hw, self.in_filter, self.crop, pix,
                         widen=self.widen, deinterlace=self.deinterlace, **({} if self.in_cube is None else {"lut": self.in_cube}),
                         **({} if self.signal is None else {"signal": self.signal}), **({} if self.pal is None else {"pal": self.pal}),
                         **({} if self.in_chroma_rows == "progressive" else {"chroma_rows": self.in_chroma_rows}))

    def delivery_end(self, device, pix):
        """The DeliveryEnd behind a chain of `pix`."""
        from .ends import DeliveryEnd
        return DeliveryEnd(device, self.render_hw, pix, self.out_pix_fmt, self.out_matrix, self.out_range, self.out_chroma, self.deliver,
                           self.deliver_filter, self.deliver_fit, self.pad_color, narrow=self.narrow,
                           **({} if self.deliver_cube is None else {"lut": self.deliver_cube}), **({} if self.weave is None else {"interlace": self.weave}),
                           **({} if self.out_chroma_rows == "progressive" else {"chroma_rows": self.out_chroma_rows}))


@dataclass(frozen=True)
class FieldChainOptions(ChainOptions):
    """The spec of a source or a delivery whose 4:2:0 chroma rows alternate between the fields: what `ChainOptions.build` returns for
    in_chroma_rows="interlaced", out_chroma_rows="interlaced" or both.  A class of its own because every defaulted field of ChainOptions
    is one that the recorded cases of tests/test_chain_options.py move; "progressive" stays the base class's constant for both."""
    in_chroma_rows: str = "interlaced"
    out_chroma_rows: str = "progressive"


@dataclass(frozen=True)
class PalChainOptions(ChainOptions):
    """The spec of a source that comes through the PAL cable: what `ChainOptions.build` returns for signal_standard="pal".  It carries the
    three values of PAL_RULES; "ntsc" stays the base class's constant, for the reason FieldChainOptions gives."""
    signal_standard: str = "pal"
    pal_decoder: str = "delay"
    signal_phase: int = 0


@dataclass(frozen=True)
class PalFieldChainOptions(FieldChainOptions):
    """Both at once — 576i 4:2:0 through the PAL cable: the fields of FieldChainOptions and those of PalChainOptions."""
    signal_standard: str = "pal"
    pal_decoder: str = "delay"
    signal_phase: int = 0
