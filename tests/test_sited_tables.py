"""The sited source stage without a GPU: the ties of tests/sited_model.py to the replicating stages' models, the tap tables written out, a
chroma ramp, the integer model against its float64 restatement, the accumulator bounds of include/crtfx_sited.h, its C-ABI bound symbol for
symbol and failing cleanly without a device, the refusals of process_frames and the CLI, and the fourteen kernel builds' registers."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pythoncrt_amd import _lib, tables  # noqa: E402
from tests import deep_model, unpack_model, yuv422_model  # noqa: E402
from tests import sited_model as model  # noqa: E402

HEADER = os.path.join(ROOT, "include", "crtfx_sited.h")


def _bits(a):
    return a.view(np.uint16) if a.dtype == np.float16 else a


# ---- ties to the replicating stages' models ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", model.LAYOUTS)
def test_literals_and_geometry_are_the_existing_families(layout):
    assert model.MATRICES8 is unpack_model.MATRICES and model.MATRICES10 is deep_model.RGB_MATRICES
    from pythoncrt_amd import sited
    for matrix, rng in model.CASES:
        m, off, top = model.tables(layout, matrix, rng)
        tm, toff = (tables.rgb_matrix10 if layout in model.DEEP else tables.rgb_matrix)(matrix, rng)
        assert np.array_equal(m.reshape(-1), tm) and tuple(toff) == tuple(off) and top == (1020 if layout in model.DEEP else 255)
    for h, w in ((1, 1), (2, 2), (3, 5), (5, 3), (16, 64), (37, 131), (1080, 1920)):
        ch, cw = (h + 1) // 2, (w + 1) // 2
        want = {"yuv420p": h * w + 2 * ch * cw, "nv12": h * w + 2 * ch * cw, "yuv422p": h * w + 2 * h * cw, "yuyv422": 4 * h * cw, "uyvy422": 4 * h * cw,
                "yuv420p10le": 2 * (h * w + 2 * ch * cw), "p010le": 2 * (h * w + 2 * ch * cw)}[layout]
        assert sited.frame_bytes(h, w, layout) == model.frame_bytes(h, w, layout) == want
    assert list(sited.LAYOUTS) == list(model.LAYOUTS) and list(sited.LAYOUTS.values()) == list(range(7))
    with pytest.raises(ValueError):
        sited.frame_bytes(4, 4, "yuv444p10le")


@pytest.mark.parametrize("siting", model.SITINGS)
@pytest.mark.parametrize("layout", model.LAYOUTS)
def test_equal_taps_give_the_replicating_stage_s_bytes(layout, siting):
    """Constant chroma planes (random luma), and every 1 x 1 and 2 x 2 frame: byte for byte the existing model of the layout's family, for
    all four matrices."""
    rs = np.random.default_rng(11)
    top = 1024 if layout in model.DEEP else 256
    for matrix, rng in model.CASES:
        for h, w in ((1, 1), (2, 2), (3, 5), (5, 3), (8, 16), (17, 33)):
            rows, cw = ((h + 1) // 2 if layout in model.V420 else h), (w + 1) // 2
            for u0, v0 in ((0, top - 1), (top - 1, 0), (int(rs.integers(top)), int(rs.integers(top)))):
                y = rs.integers(0, top, (h, w))
                p = model.pack_planes(y, np.full((rows, cw), u0), np.full((rows, cw), v0), layout)
                got, exp = model.unpack(p, h, w, layout, siting, matrix, rng), model.replicate(p, h, w, layout, matrix, rng)
                assert got.dtype == exp.dtype and np.array_equal(_bits(got), _bits(exp)), (h, w, matrix, rng, u0, v0)
        for h, w in ((1, 1), (2, 2)):
            for p in model.images(h, w, layout):
                assert np.array_equal(_bits(model.unpack(p, h, w, layout, siting, matrix, rng)), _bits(model.replicate(p, h, w, layout, matrix, rng)))


@pytest.mark.parametrize("layout", model.LAYOUTS)
def test_random_frames_differ_from_the_replicating_stage(layout):
    """The taps are live.  Where a pixel has a tap on another sample than its own (model.live) more than half of the elements of a random
    frame differ from the replicating stage's; where it has none — by the tap tables: siting "left" leaves the even columns of a 4:2:2 frame
    without one, so such a frame can never differ in more than half of its elements — they are equal.  From 8 x 16 up more than half of the
    WHOLE frame differs for every 4:2:0 layout and for siting "center"."""
    for siting in model.SITINGS:
        for h, w in ((4, 8), (8, 16), (17, 33)):
            p = model.images(h, w, layout)[0]
            each = _bits(model.unpack(p, h, w, layout, siting)) != _bits(model.replicate(p, h, w, layout))
            mask = model.live(h, w, layout, siting)
            assert not each[~mask].any() and each[mask].mean() > 0.5, (layout, siting, h, w, each[mask].mean())
            if (h, w) != (4, 8) and (layout in model.V420 or siting == "center"):
                assert 0.5 < each.mean() < 0.95, (layout, siting, h, w, each.mean())
    assert not model.live(6, 8, "uyvy422", "left")[:, 0::2].any() and model.live(6, 8, "uyvy422", "left")[:, 1:-1:2].all()
    assert model.live(6, 8, "nv12", "left")[1:-1].all() and not model.live(6, 8, "nv12", "left")[0, 0::2].any()


# ---- the taps, written out ----------------------------------------------------------------------------------------------------------------------

H_TAPS = {   # (siting, w): per column (cx, cxf, hn, hf)
    ("left", 1): [(0, 0, 4, 0)],
    ("left", 2): [(0, 0, 4, 0), (0, 0, 2, 2)],
    ("left", 5): [(0, 0, 4, 0), (0, 1, 2, 2), (1, 1, 4, 0), (1, 2, 2, 2), (2, 2, 4, 0)],
    ("left", 8): [(0, 0, 4, 0), (0, 1, 2, 2), (1, 1, 4, 0), (1, 2, 2, 2), (2, 2, 4, 0), (2, 3, 2, 2), (3, 3, 4, 0), (3, 3, 2, 2)],
    ("center", 1): [(0, 0, 3, 1)],
    ("center", 2): [(0, 0, 3, 1), (0, 0, 3, 1)],
    ("center", 5): [(0, 0, 3, 1), (0, 1, 3, 1), (1, 0, 3, 1), (1, 2, 3, 1), (2, 1, 3, 1)],
    ("center", 8): [(0, 0, 3, 1), (0, 1, 3, 1), (1, 0, 3, 1), (1, 2, 3, 1), (2, 1, 3, 1), (2, 3, 3, 1), (3, 2, 3, 1), (3, 3, 3, 1)],
}
V_TAPS = {   # h: per row (cy, cyf, vn, vf), 4:2:0
    1: [(0, 0, 3, 1)],
    3: [(0, 0, 3, 1), (0, 1, 3, 1), (1, 0, 3, 1)],
    4: [(0, 0, 3, 1), (0, 1, 3, 1), (1, 0, 3, 1), (1, 1, 3, 1)],
}


def test_tap_tables():
    for (siting, w), want in H_TAPS.items():
        got = [tuple(int(t[x]) for t in model.h_taps(w, siting)) for x in range(w)]
        # a far tap of weight 0 is never read: the model names the own sample there, as the table does
        assert got == want, (siting, w, got)
    for h, want in V_TAPS.items():
        assert [tuple(int(t[y]) for t in model.v_taps(h, True)) for y in range(h)] == want, h
        assert [tuple(int(t[y]) for t in model.v_taps(h, False)) for y in range(h)] == [(y, y, 4, 0) for y in range(h)]
    # D of single impulses: the weights of a pixel sum to 16 and land where the tables say
    for siting in model.SITINGS:
        for v420 in (True, False):
            h, w = 5, 7
            rows, cw = ((h + 1) // 2 if v420 else h), (w + 1) // 2
            total = np.zeros((h, w), dtype=np.int64)
            for r in range(rows):
                for c in range(cw):
                    imp = np.zeros((rows, cw), dtype=np.int64)
                    imp[r, c] = 1
                    total += model.interpolate(imp, h, w, siting, v420)
            assert (total == 16).all()


def test_a_linear_ramp_is_reproduced():
    """4:2:2 (no vertical taps), C[cx] = 10 + 6 cx over cw = 8: exact in the interior, the clamped taps flatten the two ends."""
    c = np.tile(10 + 6 * np.arange(8, dtype=np.int64), (3, 1))
    center = model.interpolate(c, 3, 16, "center", False) / 16.0
    left = model.interpolate(c, 3, 16, "left", False) / 16.0
    assert center[0].tolist() == [10.0, 11.5] + [14.5 + 3.0 * i for i in range(13)] + [52.0] and center[0][14] == 50.5
    assert left[0].tolist() == [10.0 + 3.0 * x for x in range(15)] + [52.0]
    assert (center == center[0]).all() and (left == left[0]).all()
    x = np.arange(1, 15)
    assert np.array_equal(center[0][1:15], 10 + 6 * (x - 0.5) / 2) and np.array_equal(left[0][:15], 10 + 6 * np.arange(15) / 2)
    # 4:2:0, a vertical ramp: rows sit at 2 cy + 0.5
    v = np.tile((20 + 8 * np.arange(4, dtype=np.int64))[:, None], (1, 4))
    d = model.interpolate(v, 8, 8, "left", True) / 16.0
    assert d[:, 0].tolist() == [20.0, 22.0, 26.0, 30.0, 34.0, 38.0, 42.0, 44.0]


# ---- the integer model against the float restatement -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("matrix,rng", model.CASES)
@pytest.mark.parametrize("layout", ("nv12", "uyvy422", "p010le"))
def test_model_against_the_float_restatement(layout, matrix, rng):
    """Random frames: the codes are the float64 ones except where the float value lies within 3 * max_sample * 2^-16 of a half-integer (the
    most three coefficients rounded to 2^-16 move a sum: the bound of the replicating stages' tests; the interpolation itself is exact in
    both), and there they differ by one."""
    bound = 3 * (1023 if layout in model.DEEP else 255) * 2.0 ** -16
    for siting in model.SITINGS:
        for h, w in ((17, 33), (32, 64)):
            for p in model.images(h, w, layout)[:2]:
                got = model.codes(p, h, w, layout, siting, matrix, rng)
                exp, raw = model.unpack_float(p, h, w, layout, siting, matrix, rng)
                d = got - exp
                assert np.abs(d).max() <= 1
                dist = np.abs(raw - np.floor(raw) - 0.5)
                assert (dist[d != 0] <= bound).all(), float(dist[d != 0].max())


# ---- accumulators ----------------------------------------------------------------------------------------------------------------------------

def _sat_add(a, b):
    return np.clip(a + b, -2 ** 31, 2 ** 31 - 1)


def test_accumulator_bounds_of_all_eight_matrices():
    """8-bit: the header's rule holds for the four matrices (at most 8.8e8).  10-bit: the whole sum passes int32 (bt601 limited range, B
    row), the luma part and the chroma part with the rounding term each fit, and a saturating 32-bit add of the two gives the int64 model's
    code at every corner of the sample cube."""
    for key, m in model.MATRICES8.items():
        for row in m:
            worst = sum(abs(c) for c in row) * 255 * 16 + (1 << 19)
            assert worst < 2 ** 31 and worst <= 8.8e8, (key, row, worst)
    over = 0
    for key, m in model.MATRICES10.items():
        off = model.OFFSETS10[key[1]]
        span = [16 * max(o, 1023 - o) for o in off]
        for row in m:
            luma, chroma = abs(row[0]) * span[0], abs(row[1]) * span[1] + abs(row[2]) * span[2] + (1 << 19)
            assert luma < 2 ** 31 and chroma < 2 ** 31, (key, row)
            over += luma + chroma >= 2 ** 31
            assert chroma <= (abs(row[1]) + abs(row[2])) * 8192 + (1 << 19) and luma <= 16 * abs(row[0]) * 1023
            for y in (0, 1023):
                for u in (0, 1023):
                    for v in (0, 1023):
                        lp, cp = 16 * row[0] * (y - off[0]), row[1] * 16 * (u - off[1]) + row[2] * 16 * (v - off[2]) + (1 << 19)
                        assert np.clip((lp + cp) >> 20, 0, 1020) == np.clip(int(_sat_add(lp, cp)) >> 20, 0, 1020)
    assert over >= 1
    b = model.MATRICES10[("bt601", "tv")][2]
    assert 16 * b[0] * (1023 - 64) + 16 * b[1] * 511 + (1 << 19) > 2.2e9


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------

def test_header_prototypes_are_the_bound_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_sited_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(_lib.SITED_SYMBOLS) and len(protos) == 7, set(protos) ^ set(_lib.SITED_SYMBOLS)
    others = (set(_lib.SYMBOLS) | set(_lib.INGEST_SYMBOLS) | set(_lib.EGRESS_SYMBOLS) | set(_lib.UNPACK_SYMBOLS) | set(_lib.DEEP_SYMBOLS) | set(_lib.YUV422_SYMBOLS)
              | set(_lib.DEEP444_SYMBOLS))
    assert not set(_lib.SITED_SYMBOLS) & others and _lib.SITED_SYMBOLS == _lib.stage_symbols("sited")
    for name, args in protos.items():
        assert len(args.split(",")) == len(_lib.SITED_SYMBOLS[name][1]), name
        assert _lib.SITED_SYMBOLS[name] == _lib.UNPACK_SYMBOLS[name.replace("crtfx_sited_", "crtfx_unpack_")], name
    enum = re.search(r"enum crtfx_sited_layout\s*\{(.*?)\}", hdr, re.S).group(1)
    assert [(n, int(v)) for n, v in re.findall(r"CRTFX_SITED_(\w+)\s*=\s*(\d+)", enum)] == [(l.upper(), i) for i, l in enumerate(model.LAYOUTS)]
    assert re.search(r"CRTFX_SITED_LEFT\s*=\s*0\s*,\s*CRTFX_SITED_CENTER\s*=\s*1", hdr)
    assert re.search(r"CRTFX_SITED_OPT_FORCE_GENERAL\s*=\s*1\s*,\s*CRTFX_SITED_OPT_SITING\s*=\s*2", hdr)
    assert (_lib.SITED_LEFT, _lib.SITED_CENTER, _lib.SITED_OPT_FORCE_GENERAL, _lib.SITED_OPT_SITING) == (0, 1, 1, 2)
    assert [getattr(_lib, "SITED_" + l.upper()) for l in model.LAYOUTS] == list(range(7))
    assert all(os.path.basename(f) in {os.path.basename(s) for s in _lib.SOURCES} for f in ("crtfx_sited.hip", "crtfx_sited.h"))
    assert "crtfx_sited" in _lib.STAGE_UNITS
    lib = _lib.load()
    for name in _lib.SITED_SYMBOLS:
        assert getattr(lib, name).argtypes == _lib.SITED_SYMBOLS[name][1]
    import pythoncrt_amd as pc
    from pythoncrt_amd import _stage
    assert pc.UnpackSited.__name__ in pc.__all__ and issubclass(pc.UnpackSited, _stage.SourcePlan)


def _create(lib, layout=_lib.SITED_NV12, h=12, w=20, pix_fmt=None, device=0, m=None, off=None, null=False, null_off=False):
    deep = layout in (_lib.SITED_YUV420P10LE, _lib.SITED_P010LE)
    tm, toff = (tables.rgb_matrix10 if deep else tables.rgb_matrix)("bt601", "tv")
    m = tm if m is None else np.ascontiguousarray(m, dtype=np.int32)
    off = toff if off is None else np.ascontiguousarray(off, dtype=np.int32)
    pix_fmt = (_lib.PIX_F16 if deep else _lib.PIX_U8) if pix_fmt is None else pix_fmt
    plan = ctypes.c_void_p(1)
    rc = lib.crtfx_sited_create(device, h, w, pix_fmt, layout, None if null else tables.ptr(m), None if null_off else tables.ptr(off), ctypes.byref(plan))
    return rc, plan, (lib.crtfx_sited_last_error(None) or b"").decode()


def test_create_refuses_bad_arguments_before_it_touches_a_device():
    """The argument checks come first, so they hold on any machine.  The pixel format follows from the layout: the other one is
    UNSUPPORTED, anything else INVALID; sizes, layouts, null tables, offsets and a matrix one step past the header's admission rule are
    INVALID; each leaves *out_plan NULL and a message.  A matrix on the rule's boundary is admitted."""
    lib = _lib.load()
    good8, good10 = tables.rgb_matrix("bt601", "tv")[0], tables.rgb_matrix10("bt601", "tv")[0]
    # 8-bit: s * 4080 + 2^19 < 2^31
    s8 = (2 ** 31 - 2 ** 19 - 1) // 4080
    assert s8 * 4080 + 2 ** 19 < 2 ** 31 <= (s8 + 1) * 4080 + 2 ** 19
    fits8, over8, split8 = good8.copy(), good8.copy(), good8.copy()
    fits8[0:3] = (s8, 0, 0)
    over8[0:3] = (s8 + 1, 0, 0)
    split8[3:6] = (s8 - 9, -5, 5)                                # the rule sums magnitudes: one past in all
    # 10-bit, offsets (64, 512, 512): 16 * 959 * |m0| < 2^31 and 8192 * (|m1| + |m2|) + 2^19 < 2^31
    l10, c10 = (2 ** 31 - 1) // (16 * 959), (2 ** 31 - 2 ** 19 - 1) // 8192
    assert 16 * 959 * l10 < 2 ** 31 <= 16 * 959 * (l10 + 1) and 8192 * c10 + 2 ** 19 < 2 ** 31 <= 8192 * (c10 + 1) + 2 ** 19
    fits10, over10l, over10c = good10.copy(), good10.copy(), good10.copy()
    fits10[0:3] = (l10, c10 - 7, -7)
    over10l[0:3] = (l10 + 1, 0, 0)
    over10c[6:9] = (0, -(c10 - 6), 7)
    cases = [(dict(pix_fmt=_lib.PIX_F16), _lib.E_UNSUPPORTED, "uint8"), (dict(layout=_lib.SITED_UYVY422, pix_fmt=_lib.PIX_F16), _lib.E_UNSUPPORTED, "uint8"),
             (dict(layout=_lib.SITED_P010LE, pix_fmt=_lib.PIX_U8), _lib.E_UNSUPPORTED, "half"),
             (dict(layout=_lib.SITED_YUV420P10LE, pix_fmt=_lib.PIX_U8), _lib.E_UNSUPPORTED, "half"),
             (dict(pix_fmt=7), _lib.E_INVALID, "pixel format"), (dict(layout=_lib.SITED_P010LE, pix_fmt=-1), _lib.E_INVALID, "pixel format"),
             (dict(h=0), _lib.E_INVALID, "size"), (dict(w=0), _lib.E_INVALID, "size"), (dict(w=32768), _lib.E_INVALID, "size"), (dict(h=32768), _lib.E_INVALID, "size"),
             (dict(layout=7), _lib.E_INVALID, "layout"), (dict(layout=-1), _lib.E_INVALID, "layout"), (dict(layout=7, pix_fmt=_lib.PIX_F16), _lib.E_INVALID, "layout"),
             (dict(null=True), _lib.E_INVALID, "null"), (dict(null_off=True), _lib.E_INVALID, "null"),
             (dict(off=(16, 256, 128)), _lib.E_INVALID, "offset"), (dict(off=(-1, 128, 128)), _lib.E_INVALID, "offset"),
             (dict(layout=_lib.SITED_P010LE, off=(64, 512, 1024)), _lib.E_INVALID, "offset"),
             (dict(m=over8), _lib.E_INVALID, "accumulator"), (dict(m=split8), _lib.E_INVALID, "accumulator"),
             (dict(layout=_lib.SITED_P010LE, m=over10l), _lib.E_INVALID, "accumulator"), (dict(layout=_lib.SITED_YUV420P10LE, m=over10c), _lib.E_INVALID, "accumulator")]
    for kw, code, word in cases:
        rc, plan, msg = _create(lib, **kw)
        assert rc == code and not plan.value and word in msg, (kw, rc, plan.value, msg)
    ok = [dict(m=fits8), dict(layout=_lib.SITED_P010LE, m=fits10), dict(h=32767, w=32767), dict(layout=_lib.SITED_P010LE, off=(64, 512, 1023), m=good10 // 2)]
    ok += [dict(layout=i) for i in range(7)]
    for kw in ok:
        rc, plan, msg = _create(lib, **kw)
        assert rc in (_lib.OK, _lib.E_HIP), (kw, rc, msg)             # no device here: E_HIP; with one: a plan
        if rc == _lib.OK:
            assert lib.crtfx_sited_destroy(plan) == _lib.OK
    assert lib.crtfx_sited_create(0, 12, 20, _lib.PIX_U8, _lib.SITED_NV12, tables.ptr(good8), tables.ptr(tables.rgb_matrix("bt601", "tv")[1]), None) == _lib.E_INVALID
    assert b"out_plan" in lib.crtfx_sited_last_error(None)
    assert lib.crtfx_sited_destroy(None) == _lib.OK and lib.crtfx_sited_set_option(None, 1, 1) == _lib.E_INVALID
    assert lib.crtfx_sited_set_option(None, 2, 1) == _lib.E_INVALID
    assert lib.crtfx_sited_run(None, None, 0, None, 0, 1, None) == _lib.E_INVALID and lib.crtfx_sited_frame_bytes(None) == 0
    assert lib.crtfx_sited_last_plan(None, ctypes.create_string_buffer(8), 8) == _lib.E_INVALID


def test_create_without_a_gpu_fails_cleanly():
    import torch
    lib = _lib.load()
    if torch.cuda.is_available():
        rc, plan, msg = _create(lib, device=4096)               # no such device on any box
        assert rc == _lib.E_HIP and not plan.value and "4096" in msg
        return
    rc, plan, msg = _create(lib)
    assert rc == _lib.E_HIP and not plan.value and msg, (rc, msg)


def test_the_class_refuses_what_needs_no_library_call():
    from pythoncrt_amd import UnpackSited
    with pytest.raises(ValueError) as e:
        UnpackSited("cuda", (8, 8), "nv12", siting="top-left")
    assert "siting" in str(e.value)
    with pytest.raises(ValueError):
        UnpackSited("cpu", (8, 8), "nv12")


# ---- refusals of process_frames and the CLI -----------------------------------------------------------------------------------------------------

def test_process_frames_refuses_in_chroma_before_it_touches_a_device():
    import pythoncrt_amd as pc

    def never():
        raise AssertionError("a frame was read")
        yield

    def call(**kw):
        return pc.process_frames(never(), lambda a: (_ for _ in ()).throw(AssertionError("written")), 64, 36, 30.0, 1, **kw)
    cases = [dict(in_chroma="top-left"), dict(in_chroma="bilinear", in_pix_fmt="nv12"), dict(in_chroma=None), dict(in_chroma="left"),
             dict(in_chroma="center", in_pix_fmt="rgb24"), dict(in_chroma="left", in_pix_fmt="yuv444p10le", out_pix_fmt="yuv444p10le"),
             dict(in_chroma="center", in_pix_fmt="gbrp10le", out_pix_fmt="p010le"), dict(in_chroma="left", in_pix_fmt="x2rgb10le", out_pix_fmt="x2rgb10le")]
    for kw in cases:
        with pytest.raises(ValueError) as e:
            call(**kw)
        assert "in_chroma" in str(e.value), (kw, str(e.value))
    for kw, word in ((dict(in_chroma="left", in_pix_fmt="p010le"), "one end"), (dict(in_chroma="left", in_pix_fmt="nv12", resize_on="host"), "host"),
                     (dict(in_chroma="center", in_pix_fmt="p010le", out_pix_fmt="p010le", in_size=(18, 32)), "in_size")):
        with pytest.raises(ValueError) as e:                        # the refusals the other tests pin stay in front of a sited source too
            call(**kw)
        assert word in str(e.value), (kw, str(e.value))


def test_cli_in_chroma_flag_and_refusals(monkeypatch, tmp_path, capsys):
    from pythoncrt_amd import cli
    parser = cli.add_input_flags(cli.add_output_flags(cli.build_parser()))
    assert parser.parse_args(["--input", "x"]).in_chroma == "replicate"
    for v in ("replicate", "left", "center"):
        assert parser.parse_args(["--input", "x", "--in-chroma", v]).in_chroma == v
    with pytest.raises(SystemExit) as e:
        parser.parse_args(["--input", "x", "--in-chroma", "top-left"])
    assert e.value.code == 2
    src = tmp_path / "in.raw"
    src.write_bytes(bytes(8 * 8 * 6))
    base = ["--input", str(src), "--output", str(tmp_path / "out.raw"), "--width", "8", "--height", "8"]
    for extra in (["--in-chroma", "left"], ["--in-chroma", "center", "--in-pix-fmt", "yuv444p10le", "--out-pix-fmt", "yuv444p10le"]):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code not in (0, None) and "--in-chroma" in str(e.value) and not (tmp_path / "out.raw").exists()
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:                            # the sharded CLI refuses the format as it does today
        cli.main(base + ["--in-pix-fmt", "nv12", "--in-chroma", "left"])
    assert "--in-pix-fmt nv12" in str(e.value) and "sharded" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(base + ["--in-chroma", "left"])
    assert "--in-chroma" in str(e.value) and not (tmp_path / "out.raw").exists()
    capsys.readouterr()


# ---- the kernel builds ----------------------------------------------------------------------------------------------------------------------------

def test_the_fourteen_kernel_builds_and_their_registers():
    """Exactly fourteen builds (seven layouts x two paths) in crtfx_sited_impl, read from the library's code objects
    (tools/kernel_resources.py): no spills, no scratch, no LDS, no AGPRs, at most 128 registers — and the VGPR counts the header states."""
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n: v for n, v in res.items() if n.startswith("crtfx_sited_impl::")}
    assert set(found) == {f"crtfx_sited_impl::k_unpack_sited<{l}, {p}>" for l in range(7) for p in (0, 1)}, sorted(found)
    text = open(HEADER).read()
    stated = {name: (int(v), int(g)) for name, v, g in re.findall(r"(\w+) (\d+) / (\d+)", text[text.index("Registers (gfx950"):text.index("no AGPRs")])}
    assert list(stated) == list(model.LAYOUTS), stated
    for name, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == 0 and v["agpr_count"] == 0 and v["vgpr_count"] + v["agpr_count"] <= 128, (name, v)
        layout, path = map(int, re.search(r"<(\d), (\d)>", name).groups())
        assert v["vgpr_count"] == stated[model.LAYOUTS[layout]][1 - path], (name, v["vgpr_count"], stated)
