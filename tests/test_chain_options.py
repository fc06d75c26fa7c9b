"""pythoncrt_amd.options: the one statement of what `process_frames` and the CLI admit and refuse around the chain.  Every message against
those of the commit before the rule table existed (tests/golden/chain_refusals.json, written by `_record` below on that commit), one
ChainOptions from both surfaces, and the ends the spec builds against literal SourceEnd / DeliveryEnd calls.  No GPU: asking for a device
fails the test."""
import dataclasses
import inspect
import json
import os

import numpy as np
import pytest
import torch

from pythoncrt_amd import (_stage, adeint, canvas, cube, deint, depth, ends, ingest, interlace, lut3d, resample, resize16,
                           signal as signal_mod)
from tests.test_chain_ends import STAGES

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "chain_refusals.json")
LUT = "look.cube"            # written into the working directory by `_lut_here`: the identity of size 2
H, W = 46, 80

# ---- the refusals ------------------------------------------------------------------------------------------------------------------------------
# (the table entry the case is for, the keywords or None, the flags or None, (height, width) of the render).  One case per entry of
# options.RULES at the least; a rule with two messages has both surfaces.  Values are what JSON holds: lists, not tuples.
SIZE = [H, W]
CASES = [
    ("resize_on", {"resize_on": "gpu"}, None, SIZE),
    ("out_pix_fmt", {"out_pix_fmt": "bgr24"}, None, SIZE),
    ("in_pix_fmt", {"in_pix_fmt": "bgr24"}, None, SIZE),
    ("in_chroma", {"in_chroma": "right"}, None, SIZE),
    ("in_chroma_format", {"in_chroma": "left"}, ["--in-chroma", "left"], SIZE),
    ("in_chroma_format", {"in_chroma": "center", "in_pix_fmt": "gbrp10le", "out_pix_fmt": "gbrp10le"},
     ["--in-chroma", "center", "--in-pix-fmt", "gbrp10le", "--out-pix-fmt", "gbrp10le"], SIZE),
    ("out_chroma", {"out_chroma": "right"}, None, SIZE),
    ("out_chroma_format", {"out_chroma": "left"}, ["--out-chroma", "left"], SIZE),
    ("in_crop", {"in_crop": [1, 2, 3]}, None, SIZE),
    ("in_crop", {"in_crop": [0, 0, 0, 5]}, None, SIZE),
    ("in_crop", {"in_crop": [0, 0, 47, 80], "in_pix_fmt": "nv12"}, None, SIZE),
    ("in_crop", {"in_crop": [0, 0, 25, 40], "in_pix_fmt": "nv12", "in_size": [24, 40]}, None, SIZE),
    (None, None, ["--in-crop-width", "81", "--in-crop-height", "46"], SIZE),
    (None, None, ["--in-crop-x", "3"], SIZE),
    ("in_crop_host", {"in_crop": [0, 0, 10, 10], "resize_on": "host"}, None, SIZE),
    ("deliver_fit", {"deliver_fit": "fill"}, None, SIZE),
    ("deliver_pad_color", {"deliver_pad_color": [0, 0, 256]}, ["--deliver-pad-color", "0,0,256"], SIZE),
    ("deliver_pad_color", {"deliver_pad_color": [0, 0]}, ["--deliver-pad-color", "black"], SIZE),
    ("chain_pix", {"chain_pix": "full"}, None, SIZE),
    ("dither", {"dither": "noise"}, None, SIZE),
    ("deinterlace", {"deinterlace": "bob"}, None, SIZE),
    ("field_order", {"field_order": "top"}, None, SIZE),
    ("deinterlace_fields", {"deinterlace_fields": "all"}, None, SIZE),
    ("deinterlace_off", {"field_order": "bff"}, ["--field-order", "bff"], SIZE),
    ("deinterlace_off", {"deinterlace_fields": "both"}, ["--deinterlace-fields", "both"], SIZE),
    ("deinterlace_host", {"deinterlace": "edge", "resize_on": "host"}, None, SIZE),
    ("deinterlace_rows", {"deinterlace": "edge", "in_pix_fmt": "nv12"}, ["--deinterlace", "edge", "--in-pix-fmt", "nv12"], [1, W]),
    ("deinterlace_rows", {"deinterlace": "adaptive", "in_size": [1, 40]}, ["--deinterlace", "adaptive"], [1, W]),
    ("dither_unused", {"dither": "ordered"}, ["--dither", "ordered"], SIZE),
    ("dither_unused", {"dither": "ordered", "chain_pix": "half", "out_pix_fmt": "p010le"},
     ["--dither", "ordered", "--chain-pix", "half", "--out-pix-fmt", "p010le"], SIZE),
    ("one_deep_end", {"in_pix_fmt": "p010le"}, ["--in-pix-fmt", "p010le"], SIZE),
    ("one_deep_end", {"out_pix_fmt": "x2rgb10le"}, ["--out-pix-fmt", "x2rgb10le"], SIZE),
    ("deep_crop", {"in_pix_fmt": "p010le", "out_pix_fmt": "p010le", "in_crop": [0, 0, 20, 40]},
     ["--in-pix-fmt", "p010le", "--out-pix-fmt", "p010le", "--in-crop-width", "40", "--in-crop-height", "20"], SIZE),
    ("deep_in_size", {"in_pix_fmt": "p010le", "out_pix_fmt": "p010le", "in_size": [20, 40]}, None, SIZE),
    ("packed_host", {"in_pix_fmt": "nv12", "resize_on": "host"}, None, SIZE),
    ("deliver_size", {"deliver_size": [1, 2, 3]}, None, SIZE),
    ("deliver_size", {"deliver_size": [0, 5]}, ["--deliver-width", "40000", "--deliver-height", "10"], SIZE),
    (None, None, ["--deliver-width", "40"], SIZE),
    ("in_filter", {"in_filter": "nearest"}, None, SIZE),
    ("deliver_filter", {"deliver_filter": "nearest"}, None, SIZE),
    ("deliver_filter_unused", {"deliver_filter": "lanczos"}, ["--deliver-filter", "lanczos"], SIZE),
    ("deliver_filter_unused", {"deliver_filter": "box", "deliver_size": [H, W]},
     ["--deliver-filter", "box", "--deliver-width", str(W), "--deliver-height", str(H)], SIZE),
    ("deliver_fit_unused", {"deliver_fit": "pad"}, ["--deliver-fit", "pad"], SIZE),
    ("deliver_interlace", {"deliver_interlace": "on"}, None, SIZE),
    ("deliver_lowpass", {"deliver_lowpass": "soft"}, None, SIZE),
    ("deliver_lowpass_unused", {"deliver_lowpass": "linear"}, ["--deliver-lowpass", "linear"], SIZE),
    ("weave_rows", {"deliver_interlace": "tff", "deliver_size": [1, W]},
     ["--deliver-interlace", "tff", "--deliver-width", str(W), "--deliver-height", "1"], SIZE),
    ("weave_rows", {"deliver_interlace": "bff"}, ["--deliver-interlace", "bff"], [1, W]),
    ("in_signal", {"in_signal": "ntsc"}, None, SIZE),
    ("in_signal", {"in_signal": None}, None, SIZE),
    ("signal_chroma", {"signal_chroma": "blurry"}, None, SIZE),
    ("signal_crawl", {"signal_crawl": "on"}, None, SIZE),
    ("signal_off", {"signal_chroma": "soft"}, ["--signal-chroma", "soft"], SIZE),
    ("signal_off", {"signal_crawl": False}, ["--signal-crawl", "off"], SIZE),
    ("signal_host", {"in_signal": "composite", "resize_on": "host"}, None, SIZE),
    ("in_lut_host", {"in_lut": "x.cube", "resize_on": "host"}, None, SIZE),
    ("in_lut", {"in_lut": 5}, None, SIZE),
    ("in_lut", {"in_lut": "no_such.cube"}, ["--in-lut", "no_such.cube"], SIZE),
    ("deliver_lut", {"deliver_lut": 5}, None, SIZE),
    ("deliver_lut", {"deliver_lut": "no_such.cube"}, ["--deliver-lut", "no_such.cube"], SIZE),
]


def _surfaces(monkeypatch, tmp_path):
    """(keywords, size) -> the ValueError's text; (flags, size) -> the SystemExit's text.  A frame read, a device asked for or an output
    file opened fails the test (the `_refusing_process_frames` of test_signal_tables.py, for both surfaces)."""
    import pythoncrt_amd as pc
    from pythoncrt_amd import cli

    def never():
        raise AssertionError("a frame was read")
        yield

    def no_device():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("CRTFX_FORCE_DIST", raising=False)
    monkeypatch.chdir(tmp_path)                          # "no_such.cube" is looked for here
    out = tmp_path / "out.raw"

    def keywords(kw, size):
        with pytest.raises(ValueError) as e:
            pc.process_frames(never(), lambda a: None, size[1], size[0], 30.0, 1, **kw)
        return str(e.value), getattr(e.value, "rule", None)

    def flags(argv, size):
        with pytest.raises(SystemExit) as e:
            cli.main(["--input", str(tmp_path / "in.raw"), "--output", str(out), "--width", str(size[1]), "--height", str(size[0])] + argv)
        assert not out.exists() and isinstance(e.value.code, str)
        return e.value.code, getattr(e.value.__cause__, "rule", None)
    return keywords, flags


def _record(monkeypatch, tmp_path):
    """Writes the golden file: run once, through pytest's fixtures, on the commit whose messages are the reference (not collected)."""
    keywords, flags = _surfaces(monkeypatch, tmp_path)
    rows = [{"rule": rule, "size": size, "keywords": kw, "error": None if kw is None else keywords(kw, size)[0],
             "argv": argv, "exit": None if argv is None else flags(argv, size)[0]} for rule, kw, argv, size in CASES]
    with open(GOLDEN, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


def test_every_refusal_keeps_the_text_it_had(monkeypatch, tmp_path):
    """Every recorded case, on both surfaces where it has both: the same text, raised by the table entry the case names — and between them
    the cases fire every entry of the table on every surface the entry speaks on."""
    from pythoncrt_amd import options
    keywords, flags = _surfaces(monkeypatch, tmp_path)
    rows = json.load(open(GOLDEN))
    assert [(r["rule"], r["keywords"], r["argv"], r["size"]) for r in rows] == [tuple(c) for c in CASES]     # no case left out
    by_name = {r.name: r for r in options.RULES}
    assert len(by_name) == len(options.RULES)
    fired = set()
    for r in rows:
        rule = by_name.get(r["rule"])
        if r["keywords"] is not None:
            assert keywords(r["keywords"], r["size"]) == (r["error"], r["rule"]), r
            fired.add((r["rule"], "keywords"))
        if r["argv"] is not None:
            on_flags = rule is not None and rule.flags is not None        # else: argparse's, or a parser of cli.py
            assert flags(r["argv"], r["size"]) == (r["exit"], r["rule"] if on_flags else None), r
            fired |= {(r["rule"], "flags")} if on_flags else set()
    assert fired == {(r.name, s) for r in options.RULES for s in ("keywords", "flags") if getattr(r, s) is not None}


# ---- what is admitted ----------------------------------------------------------------------------------------------------------------------------
# (keywords, the same as flags or None where the CLI cannot say it).  The CLI reads its input at render size: in_size is the render size there
ADMITTED = [
    ({}, []),
    ({"in_signal": "composite"}, ["--in-signal", "composite"]),
    ({"in_signal": "svideo", "signal_chroma": "soft", "signal_crawl": False}, ["--in-signal", "svideo", "--signal-chroma", "soft", "--signal-crawl", "off"]),
    ({"in_signal": "rgb"}, ["--in-signal", "rgb"]),
    ({"in_signal": "rgb", "signal_chroma": "sharp", "signal_crawl": True, "resize_on": "host"}, None),
    ({"in_signal": "composite", "in_pix_fmt": "uyvy422", "in_size": (48, 72), "deinterlace": "edge", "deinterlace_fields": "both"}, None),
    ({"in_signal": "composite", "in_pix_fmt": "uyvy422", "deinterlace": "edge", "deinterlace_fields": "both"},
     ["--in-signal", "composite", "--in-pix-fmt", "uyvy422", "--deinterlace", "edge", "--deinterlace-fields", "both"]),
    ({"in_signal": "composite", "chain_pix": "half", "in_pix_fmt": "nv12", "in_size": (30, 40), "in_filter": "lanczos"}, None),
    ({"in_signal": "composite", "chain_pix": "half", "in_pix_fmt": "nv12", "in_filter": "lanczos"},
     ["--in-signal", "composite", "--chain-pix", "half", "--in-pix-fmt", "nv12", "--in-filter", "lanczos"]),
    ({"in_signal": "svideo", "in_pix_fmt": "p010le", "out_pix_fmt": "yuv444p10le", "signal_chroma": "soft"},
     ["--in-signal", "svideo", "--in-pix-fmt", "p010le", "--out-pix-fmt", "yuv444p10le", "--signal-chroma", "soft"]),
    ({"in_pix_fmt": "yuv420p", "in_matrix": "bt709", "in_range": "pc", "in_chroma": "left"},
     ["--in-pix-fmt", "yuv420p", "--in-matrix", "bt709", "--in-range", "pc", "--in-chroma", "left"]),
    ({"out_pix_fmt": "nv12", "out_matrix": "bt709", "out_range": "pc", "out_chroma": "left"},
     ["--out-pix-fmt", "nv12", "--out-matrix", "bt709", "--out-range", "pc", "--out-chroma", "left"]),
    ({"in_crop": (2, 4, 40, 60)}, ["--in-crop-y", "2", "--in-crop-x", "4", "--in-crop-height", "40", "--in-crop-width", "60"]),
    ({"in_pix_fmt": "gbrp10le", "out_pix_fmt": "x2rgb10le", "in_crop": (0, 0, H, W)},
     ["--in-pix-fmt", "gbrp10le", "--out-pix-fmt", "x2rgb10le", "--in-crop-height", str(H), "--in-crop-width", str(W)]),
    ({"deinterlace": "linear"}, ["--deinterlace", "linear"]),
    ({"deinterlace": "adaptive", "field_order": "bff", "deinterlace_fields": "both"},
     ["--deinterlace", "adaptive", "--field-order", "bff", "--deinterlace-fields", "both"]),
    ({"in_lut": LUT}, ["--in-lut", LUT]),
    ({"deliver_lut": LUT, "chain_pix": "half", "dither": "ordered"}, ["--deliver-lut", LUT, "--chain-pix", "half", "--dither", "ordered"]),
    ({"chain_pix": "half", "in_pix_fmt": "p010le", "out_pix_fmt": "yuv420p", "dither": "ordered"},
     ["--chain-pix", "half", "--in-pix-fmt", "p010le", "--out-pix-fmt", "yuv420p", "--dither", "ordered"]),
    ({"chain_pix": "half", "out_pix_fmt": "p010le"}, ["--chain-pix", "half", "--out-pix-fmt", "p010le"]),
    ({"deliver_size": (23, 40)}, ["--deliver-height", "23", "--deliver-width", "40"]),
    ({"deliver_size": (H, W)}, ["--deliver-height", str(H), "--deliver-width", str(W)]),
    ({"deliver_size": (23, 40), "deliver_filter": "lanczos", "out_pix_fmt": "yuv422p"},
     ["--deliver-height", "23", "--deliver-width", "40", "--deliver-filter", "lanczos", "--out-pix-fmt", "yuv422p"]),
    ({"deliver_size": (40, 40), "deliver_fit": "pad", "deliver_pad_color": (16, 128, 255)},
     ["--deliver-height", "40", "--deliver-width", "40", "--deliver-fit", "pad", "--deliver-pad-color", "16,128,255"]),
    ({"deliver_size": (40, 40), "deliver_fit": "crop", "chain_pix": "half"},
     ["--deliver-height", "40", "--deliver-width", "40", "--deliver-fit", "crop", "--chain-pix", "half"]),
    ({"deliver_interlace": "tff"}, ["--deliver-interlace", "tff"]),
    ({"deliver_interlace": "bff", "deliver_lowpass": "complex", "deliver_size": (24, 40), "deinterlace": "edge", "deinterlace_fields": "both"},
     ["--deliver-interlace", "bff", "--deliver-lowpass", "complex", "--deliver-height", "24", "--deliver-width", "40", "--deinterlace", "edge",
      "--deinterlace-fields", "both"]),
    ({"in_filter": "bicubic", "resize_on": "host"}, None),
    ({"in_pix_fmt": "p010le", "out_pix_fmt": "p010le", "in_chroma": "center", "out_chroma": "left", "in_lut": LUT, "deliver_lut": LUT,
      "deliver_size": (92, 160), "deliver_interlace": "tff", "deliver_lowpass": "linear"},
     ["--in-pix-fmt", "p010le", "--out-pix-fmt", "p010le", "--in-chroma", "center", "--out-chroma", "left", "--in-lut", LUT, "--deliver-lut", LUT,
      "--deliver-height", "92", "--deliver-width", "160", "--deliver-interlace", "tff", "--deliver-lowpass", "linear"]),
]


def _lut_here(monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    (tmp_path / LUT).write_text("LUT_3D_SIZE 2\n" + "".join(f"{r} {g} {b}\n" for b in (0, 1) for g in (0, 1) for r in (0, 1)))


KEYWORDS = ("resize_on", "out_pix_fmt", "out_matrix", "out_range", "in_pix_fmt", "in_matrix", "in_range", "in_size", "in_chroma", "out_chroma",
            "deliver_size", "in_filter", "deliver_filter", "in_crop", "deliver_fit", "deliver_pad_color", "chain_pix", "dither", "deinterlace",
            "field_order", "deinterlace_fields", "in_lut", "deliver_lut", "deliver_interlace", "deliver_lowpass", "in_signal", "signal_chroma",
            "signal_crawl")


def _from_keywords(kw):
    """The spec of process_frames(..., W, H, ..., **kw): every keyword the spec reads, at the default of process_frames' signature unless given."""
    import pythoncrt_amd as pc
    from pythoncrt_amd import options
    defaults = inspect.signature(pc.process_frames).parameters
    assert set(kw) <= set(KEYWORDS)
    return options.ChainOptions.build(options.Raw(render_hw=(H, W), **{n: kw.get(n, defaults[n].default) for n in KEYWORDS}), "keywords")


def _same(a, b):
    """Field for field; two Cubes read from the same file are the same cube."""
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, cube.Cube) and isinstance(y, cube.Cube):
            assert x.size == y.size and np.array_equal(x.values, y.values), f.name
        else:
            assert x == y and type(x) is type(y), (f.name, x, y)


def test_one_spec_from_both_surfaces(monkeypatch, tmp_path):
    from pythoncrt_amd import cli, options
    _lut_here(monkeypatch, tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("CRTFX_FORCE_DIST", raising=False)
    assert len(ADMITTED) >= 24
    parse = cli.add_input_flags(cli.add_output_flags(cli.build_parser())).parse_args
    base = ["--input", str(tmp_path / "in.raw"), "--output", str(tmp_path / "out.raw"), "--width", str(W), "--height", str(H)]
    defaults = {f.name: f.default for f in dataclasses.fields(options.ChainOptions) if f.default is not dataclasses.MISSING}
    assert set(defaults) == {f.name for f in dataclasses.fields(options.ChainOptions)} - {"render_hw"}
    moved = set()
    for kw, argv in ADMITTED:
        spec = _from_keywords(kw)
        assert spec.render_hw == (H, W)
        moved |= {name for name, value in defaults.items() if getattr(spec, name) != value}
        if argv is not None:
            flagged, ranks = cli.check_flags(parse(base + argv))
            assert ranks is None and flagged.in_size == (H, W)
            _same(_from_keywords({"in_size": (H, W), **kw}), flagged)
    assert moved == set(defaults), set(defaults) - moved
    assert not (tmp_path / "out.raw").exists()


# ---- the ends the spec builds ------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def built(monkeypatch):
    """test_chain_ends.py's recorders, over the frame-stage and resize classes too: (class, positional arguments, keywords) instead of a plan."""
    log = []
    frame_stages = [signal_mod.Signal, deint.Deinterlace, adeint.AdaptiveDeinterlace, canvas.Canvas, depth.Widen, depth.Narrow, lut3d.Lut3D,
                    interlace.Interlace]
    for cls in STAGES + [ingest.IngestResize, resize16.ResizeHalf, resample.Resample] + frame_stages:
        def init(self, *args, _cls=cls, **kw):
            log.append((_cls, args, kw))
            if issubclass(_cls, _stage.StagePlan):
                self.frame_bytes = _cls._frame_bytes(args[1][0], args[1][1], kw["layout"])
        monkeypatch.setattr(cls, "__init__", init)
    return log


def test_the_ends_the_spec_builds(built, monkeypatch, tmp_path):
    """spec.source_end / spec.delivery_end against the literal calls cli.main made before the spec existed, written out here: the same plan
    classes, positional arguments and keywords, in the same order; and spec.direct exactly where that code built no source end."""
    SourceEnd, DeliveryEnd, depth_stages = ends.SourceEnd, ends.DeliveryEnd, ends.depth_stages
    _lut_here(monkeypatch, tmp_path)
    dev = "dev"
    h, w = H, W
    for kw, _ in ADMITTED:
        spec = _from_keywords(kw)
        get = lambda name, default: kw.get(name, default)                                                   # noqa: E731
        in_pix_fmt, in_matrix, in_range, in_chroma = get("in_pix_fmt", "rgb24"), get("in_matrix", "bt601"), get("in_range", "tv"), get("in_chroma", "replicate")
        out_pix_fmt, out_matrix, out_range, out_chroma = get("out_pix_fmt", "rgb24"), get("out_matrix", "bt601"), get("out_range", "tv"), get("out_chroma", "center")
        in_filter, deliver_filter, deliver_fit, pad_color = get("in_filter", "bilinear"), get("deliver_filter", "bilinear"), get("deliver_fit", "stretch"), get("deliver_pad_color", (0, 0, 0))
        deliver = None if get("deliver_size", (h, w)) == (h, w) else kw["deliver_size"]
        crop, src_hw = get("in_crop", None), get("in_size", (h, w))
        deint = None if "deinterlace" not in kw else (kw["deinterlace"], get("field_order", "tff"), get("deinterlace_fields", "first"))
        cable = None if get("in_signal", "rgb") == "rgb" else (kw["in_signal"], get("signal_chroma", "sharp"), get("signal_crawl", True))
        weave = None if "deliver_interlace" not in kw else (kw["deliver_interlace"], get("deliver_lowpass", "none"))
        in_cube, deliver_cube = spec.in_cube, spec.deliver_cube
        assert (in_cube is None) == ("in_lut" not in kw) and (deliver_cube is None) == ("deliver_lut" not in kw)
        on_half, widen, narrow = depth_stages(in_pix_fmt, out_pix_fmt, get("chain_pix", "auto"), get("dither", "none"))
        assert (spec.half, spec.widen, spec.narrow) == (on_half, widen, narrow)
        pix = torch.float16 if on_half else torch.uint8

        del built[:]
        end = DeliveryEnd(dev, (h, w), pix, out_pix_fmt, out_matrix, out_range, out_chroma, deliver, deliver_filter, deliver_fit, pad_color,
                          narrow=narrow, **({} if deliver_cube is None else {"lut": deliver_cube}), **({} if weave is None else {"interlace": weave}))
        source = (SourceEnd(dev, (h, w), in_pix_fmt, in_matrix, in_range, in_chroma, src_hw, in_filter, crop, pix, widen=widen, deinterlace=deint,
                            **({} if in_cube is None else {"lut": in_cube}), **({} if cable is None else {"signal": cable}))
                  if in_pix_fmt != "rgb24" or crop is not None or widen or deint is not None or in_cube is not None or cable is not None else None)
        literal = list(built)
        assert spec.direct is (source is None), kw

        del built[:]
        end2 = spec.delivery_end(dev, pix)
        source2 = None if spec.direct else spec.source_end(dev, src_hw, pix)
        assert built == literal, (kw, built, literal)
        assert type(end2) is DeliveryEnd and (end2.size, end2.frame_bytes, len(end2.stages)) == (end.size, end.frame_bytes, len(end.stages))
        if source is not None:
            assert type(source2) is SourceEnd
            assert (source2.src_hw, source2.frame_bytes, source2.ratio, len(source2.stages)) == (source.src_hw, source.frame_bytes, source.ratio, len(source.stages))
        B = 7
        want = max(2, B - B % 2) if weave is not None or (deint is not None and deint[2] == "both") else B
        assert spec.ratio == (source.ratio if source is not None else 1) and spec.batch(B) == (want, want // spec.ratio)
        assert spec.batch(0) == spec.batch(1)
