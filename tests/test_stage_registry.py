"""The one format registry (pythoncrt_amd/formats.py) against the CLI's flags and the family modules, and the generated ctypes tables of the
format stages (_lib.stage_symbols) against the seven entry points written out; the same for the resize stages (_lib.resize_symbols) and the
frame stages (_lib.frame_symbols).  No GPU."""
import argparse
import ctypes

import pytest

from pythoncrt_amd import _lib, cli, deep, deep444, egress, formats, unpack, yuv422

SIZES = [(1, 1), (2, 8), (3, 5), (1080, 1920)]


def _choices(add_flags, flag):
    parser = add_flags(argparse.ArgumentParser())
    return next(a.choices for a in parser._actions if flag in a.option_strings)


def test_the_cli_accepts_exactly_the_registry():
    """Every name --in-pix-fmt / --out-pix-fmt accept is a registry entry (or rgb24, the chain's own format, which needs no stage), and
    every registry entry is accepted on both ends; process_frames takes the same names."""
    for got in (_choices(cli.add_input_flags, "--in-pix-fmt"), _choices(cli.add_output_flags, "--out-pix-fmt"), cli.IN_PIX_FMTS, cli.OUT_PIX_FMTS):
        assert len(got) == len(set(got)) and set(got) - {"rgb24"} == set(formats.FORMATS) and "rgb24" in got, got
    assert "rgb24" not in formats.FORMATS and formats.PIX_FMTS == ("rgb24",) + tuple(formats.FORMATS)
    assert set(formats.FORMATS) == {"yuv420p", "nv12", "yuv422p", "yuyv422", "uyvy422", "yuv420p10le", "p010le", "yuv444p10le", "gbrp10le", "x2rgb10le"}
    assert cli.DEEP_PIX_FMTS + cli.DEEP444_PIX_FMTS == tuple(f for f in formats.FORMATS if formats.bits(f) == 10)
    assert formats.bits("rgb24") == 8 and all(formats.bits(f) == 8 for f in ("yuv420p", "nv12") + cli.YUV422_PIX_FMTS)


def test_every_format_names_its_family():
    """The classes and the sample depth of each entry: the source and egress plan of the family module that lists the format."""
    modules = {unpack: (unpack.UnpackYuv, egress.EgressYuv, egress.LAYOUTS, 8), yuv422: (yuv422.UnpackYuv422, yuv422.EgressYuv422, yuv422.LAYOUTS, 8),
               deep: (deep.UnpackYuv10, deep.EgressYuv10, deep.LAYOUTS, 10), deep444: (deep444.UnpackDeep444, deep444.EgressDeep444, deep444.FORMATS, 10)}
    seen = []
    for source, sink, names, bits in modules.values():
        for name in names:
            fam = formats.FORMATS[name]
            assert (fam.source, fam.egress, fam.bits) == (source, sink, bits) and name in fam.names, name
            assert name in source._layouts and name in sink._layouts
            seen.append(name)
    assert sorted(seen) == sorted(formats.FORMATS)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frame_bytes_are_the_family_modules(size):
    h, w = size
    for fmt in ("yuv420p", "nv12"):
        assert formats.frame_bytes(h, w, fmt) == egress.frame_bytes(h, w) == unpack.frame_bytes(h, w) == formats.FORMATS[fmt].frame_bytes(h, w, fmt)
    for fmt in yuv422.LAYOUTS:
        assert formats.frame_bytes(h, w, fmt) == yuv422.frame_bytes(h, w, fmt) == formats.FORMATS[fmt].frame_bytes(h, w, fmt)
    for fmt in deep.LAYOUTS:
        assert formats.frame_bytes(h, w, fmt) == deep.frame_bytes(h, w) == formats.FORMATS[fmt].frame_bytes(h, w, fmt)
    for fmt in deep444.FORMATS:
        assert formats.frame_bytes(h, w, fmt) == deep444.frame_bytes(h, w, fmt) == formats.FORMATS[fmt].frame_bytes(h, w, fmt)
    assert formats.frame_bytes(h, w, "rgb24") == h * w * 3
    ch, cw = (h + 1) // 2, (w + 1) // 2                                        # ... and the sizes themselves, written out
    assert formats.frame_bytes(h, w, "nv12") == h * w + 2 * ch * cw and formats.frame_bytes(h, w, "p010le") == 2 * (h * w + 2 * ch * cw)
    assert formats.frame_bytes(h, w, "yuv422p") == h * w + 2 * h * cw and formats.frame_bytes(h, w, "uyvy422") == 4 * h * cw
    assert formats.frame_bytes(h, w, "gbrp10le") == 6 * h * w and formats.frame_bytes(h, w, "x2rgb10le") == 4 * h * w


def _literal(fam):
    vp = ctypes.c_void_p
    return {
        f"crtfx_{fam}_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.POINTER(vp)]),
        f"crtfx_{fam}_destroy": (ctypes.c_int, [vp]),
        f"crtfx_{fam}_last_error": (ctypes.c_char_p, [vp]),
        f"crtfx_{fam}_frame_bytes": (ctypes.c_size_t, [vp]),
        f"crtfx_{fam}_run": (ctypes.c_int, [vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, ctypes.c_int, vp]),
        f"crtfx_{fam}_set_option": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int]),
        f"crtfx_{fam}_last_plan": (ctypes.c_int, [vp, ctypes.c_char_p, ctypes.c_size_t]),
    }


@pytest.mark.parametrize("table,families", [("EGRESS_SYMBOLS", ("egress",)), ("UNPACK_SYMBOLS", ("unpack",)), ("DEEP_SYMBOLS", ("unpack10", "egress10")),
                                            ("YUV422_SYMBOLS", ("unpack422", "egress422")), ("DEEP444_SYMBOLS", ("unpack444", "egress444"))])
def test_generated_symbol_tables_equal_the_literal_seven(table, families):
    want = {}
    for fam in families:
        want.update(_literal(fam))
    got = getattr(_lib, table)
    assert got == want and len(got) == 7 * len(families) and list(got) == list(want)
    assert got == _lib.stage_symbols(*families)
    for fam in families:                                                       # the classes call exactly these families
        users = [c for f in formats.FORMATS.values() for c in (f.source, f.egress) if c._family == fam]
        assert users, fam


def _literal_resize(fam):
    vp = ctypes.c_void_p
    return {
        f"crtfx_{fam}_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_int,
                                               vp, vp, vp, ctypes.c_int, ctypes.POINTER(vp)]),
        f"crtfx_{fam}_destroy": (ctypes.c_int, [vp]),
        f"crtfx_{fam}_last_error": (ctypes.c_char_p, [vp]),
        f"crtfx_{fam}_run": (ctypes.c_int, [vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, ctypes.c_int, vp]),
        f"crtfx_{fam}_set_option": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int]),
        f"crtfx_{fam}_last_plan": (ctypes.c_int, [vp, ctypes.c_char_p, ctypes.c_size_t]),
    }


@pytest.mark.parametrize("table,family,cls,option", [("INGEST_SYMBOLS", "ingest", "IngestResize", "INGEST_OPT_FORCE_GENERAL"),
                                                     ("RESIZE16_SYMBOLS", "resize16", "ResizeHalf", "RESIZE16_OPT_FORCE_GENERAL"),
                                                     ("RESAMPLE_SYMBOLS", "resample", "Resample", "RESAMPLE_OPT_FORCE_GENERAL")])
def test_generated_resize_symbol_tables_equal_the_literal_six(table, family, cls, option):
    """_lib.resize_symbols against the six entry points of a resize stage written out, contents and order; _lib.load() binds them; the
    plan class calls exactly this family, and its force option is the family's *_OPT_FORCE_GENERAL."""
    import pythoncrt_amd as pc
    from pythoncrt_amd import _stage
    want = _literal_resize(family)
    got = getattr(_lib, table)
    assert got == want and len(got) == 6 and list(got) == list(want)
    assert got == _lib.resize_symbols(family)
    assert list(_lib.resize_symbols("ingest", "resample")) == list(_literal_resize("ingest")) + list(_literal_resize("resample"))
    lib = _lib.load()
    for name, (res, args) in want.items():
        assert getattr(lib, name).restype == res and getattr(lib, name).argtypes == args, name
    plan = getattr(pc, cls)
    assert issubclass(plan, _stage.ResizePlan) and issubclass(plan, _stage.Handle) and not issubclass(plan, _stage.StagePlan)
    assert plan._family == family and plan._force_option == 1 == getattr(_lib, option)


@pytest.mark.parametrize("family,pix,filter", [("ingest", _lib.PIX_U8, "bilinear"), ("resize16", _lib.PIX_F16, "bilinear"),
                                               ("resample", _lib.PIX_U8, "bicubic"), ("resample", _lib.PIX_F16, "bicubic")])
def test_the_tall_case_of_the_resize_api_test_passes_the_table_checks(family, pix, filter):
    """2048 x 4 -> 1 x 4, the pair tests/test_resize_api_gpu.py takes for the general path by necessity: its tables pass every check of
    crtfx_<family>_create (the call gets as far as the device, and device 4096 exists on no machine), and each row of the 2048 the one
    output row reaches costs at least 32 bytes of LDS, more than the budget of 40 960 bytes for any tile shape."""
    from pythoncrt_amd import tables
    src, dst = (2048, 4), (1, 4)
    axis = tables.pil_resample_axis if filter == "bilinear" else (lambda a, b: tables.pil_filter_axis(a, b, filter))
    ax, ay = axis(src[1], dst[1]), axis(src[0], dst[0])
    assert int(ay[0][0]) == 0 and int(ay[1][0]) == 2048 and 2048 * 32 > 40960
    lib = _lib.load()
    plan = ctypes.c_void_p(1)
    rc = getattr(lib, f"crtfx_{family}_create")(4096, src[0], src[1], dst[0], dst[1], pix, tables.ptr(ax[0]), tables.ptr(ax[1]), tables.ptr(ax[2]), ax[2].shape[1],
                                                tables.ptr(ay[0]), tables.ptr(ay[1]), tables.ptr(ay[2]), ay[2].shape[1], ctypes.byref(plan))
    msg = (getattr(lib, f"crtfx_{family}_last_error")(None) or b"").decode()
    assert rc == _lib.E_HIP and not plan.value and msg == "no HIP device 4096", (rc, msg)


_FRAME_OWN = {        # family -> (create's own arguments behind `device`, the entry points beside the shared five)
    "canvas": ([ctypes.c_int] * 11 + [ctypes.POINTER(ctypes.c_uint16)], {}),
    "depth": ([ctypes.c_int] * 4, {}),
    "deint": ([ctypes.c_int] * 6, {"frames_out": (ctypes.c_int, [ctypes.c_void_p])}),
    "adeint": ([ctypes.c_int] * 5, {"frames_out": (ctypes.c_int, [ctypes.c_void_p]),
                                    "run": (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                                           ctypes.c_void_p])}),
    "lut3d": ([ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_uint16)],
              {"set_table": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_uint16)])}),
}


def _literal_frame(fam):
    vp = ctypes.c_void_p
    create_args, extra = _FRAME_OWN[fam]
    table = {
        f"crtfx_{fam}_create": (ctypes.c_int, [ctypes.c_int] + create_args + [ctypes.POINTER(vp)]),
        f"crtfx_{fam}_destroy": (ctypes.c_int, [vp]),
        f"crtfx_{fam}_last_error": (ctypes.c_char_p, [vp]),
        f"crtfx_{fam}_run": (ctypes.c_int, [vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, ctypes.c_int, vp]),
        f"crtfx_{fam}_set_option": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int]),
        f"crtfx_{fam}_last_plan": (ctypes.c_int, [vp, ctypes.c_char_p, ctypes.c_size_t]),
    }
    for name, sig in extra.items():                                            # a further entry point goes behind the six; the family's own run stays in run's place
        table[f"crtfx_{fam}_{name}"] = sig
    return table


@pytest.mark.parametrize("table,family,classes,option", [("CANVAS_SYMBOLS", "canvas", ("Canvas",), "CANVAS_OPT_FORCE_GENERAL"),
                                                         ("DEPTH_SYMBOLS", "depth", ("Widen", "Narrow"), "DEPTH_OPT_FORCE_GENERAL"),
                                                         ("DEINT_SYMBOLS", "deint", ("Deinterlace",), "DEINT_OPT_FORCE_GENERAL"),
                                                         ("ADEINT_SYMBOLS", "adeint", ("AdaptiveDeinterlace",), "ADEINT_OPT_FORCE_GENERAL"),
                                                         ("LUT3D_SYMBOLS", "lut3d", ("Lut3D",), "LUT3D_OPT_FORCE_GENERAL")])
def test_generated_frame_symbol_tables_equal_the_literal(table, family, classes, option):
    """_lib.frame_symbols against the entry points of a frame stage written out, contents and order (the SIGNATURES of the five
    test_*_tables.py files are the same tables, each beside its header); _lib.load() binds them; the plan classes stand on FramePlan and on
    neither of the other two bases, call exactly this family, and their force option is the family's *_OPT_FORCE_GENERAL."""
    import pythoncrt_amd as pc
    from pythoncrt_amd import _stage
    create_args, extra = _FRAME_OWN[family]
    want = _literal_frame(family)
    got = getattr(_lib, table)
    assert got == want and len(got) == 6 + len([k for k in extra if k != "run"]) and list(got) == list(want)
    assert got == _lib.frame_symbols(family, create_args, **extra) and list(got) == list(_lib.frame_symbols(family, create_args, **extra))
    lib = _lib.load()
    for name, (res, args) in want.items():
        assert getattr(lib, name).restype == res and getattr(lib, name).argtypes == args, name
    for cls in classes:
        plan = getattr(pc, cls)
        assert issubclass(plan, _stage.FramePlan) and issubclass(plan, _stage.Handle)
        assert not issubclass(plan, _stage.StagePlan) and not issubclass(plan, _stage.ResizePlan)
        assert plan._family == family and plan._force_option == 1 == getattr(_lib, option)
    names = [s.rsplit("/", 1)[-1] for s in _lib.SOURCES]                     # the rebuild check reads the skeleton
    assert "crtfx_frame_host.h" in names and f"crtfx_{family}.hip" in names
