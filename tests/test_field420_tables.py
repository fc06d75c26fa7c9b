"""The field-paired 4:2:0 source stage without a GPU: the vertical taps of tests/field420_model.py as literals, its ties to the replicating
stages' models (the weave of the two fields, constant chroma), a vertical chroma ramp at MPEG-2's interlaced siting, the independence of
the two fields, the integer model against its float64 restatement, the accumulator bounds of include/crtfx_field420.h, its C ABI bound
symbol for symbol and failing cleanly without a device, the refusals of process_frames, probe_frames and both CLIs, the plans SourceEnd
builds, and the eight kernel builds' registers."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pythoncrt_amd import _lib, _stage, tables  # noqa: E402
from tests import deep_model, sited_model, unpack_model  # noqa: E402
from tests import field420_model as model  # noqa: E402

HEADER = os.path.join(ROOT, "include", "crtfx_field420.h")
FOUR = "(yuv420p, nv12, yuv420p10le, p010le)"


def _bits(a):
    return a.view(np.uint16) if a.dtype == np.float16 else a


# ---- the taps, written out ----------------------------------------------------------------------------------------------------------------------

V_TAPS = {   # h: per luma row (cy, cyf, vn, vf), FRAME chroma rows, chroma "left" / "center"
    4: [(0, 0, 7, 1), (1, 1, 5, 3), (0, 0, 5, 3), (1, 1, 7, 1)],
    6: [(0, 0, 7, 1), (1, 1, 5, 3), (0, 2, 5, 3), (1, 1, 7, 1), (2, 0, 7, 1), (1, 1, 5, 3)],
    8: [(0, 0, 7, 1), (1, 1, 5, 3), (0, 2, 5, 3), (1, 3, 7, 1), (2, 0, 7, 1), (3, 1, 5, 3), (2, 2, 5, 3), (3, 3, 7, 1)],
    12: [(0, 0, 7, 1), (1, 1, 5, 3), (0, 2, 5, 3), (1, 3, 7, 1), (2, 0, 7, 1), (3, 1, 5, 3), (2, 4, 5, 3), (3, 5, 7, 1), (4, 2, 7, 1), (5, 3, 5, 3),
         (4, 4, 5, 3), (5, 5, 7, 1)],
}


def test_tap_tables():
    for h, want in V_TAPS.items():
        for chroma in ("left", "center"):
            assert [tuple(int(t[y]) for t in model.v_taps(h, chroma)) for y in range(h)] == want, (h, chroma)
        cy, cyf, vn, vf = model.v_taps(h, "replicate")
        assert cy.tolist() == [row[0] for row in want] and cyf.tolist() == [row[1] for row in want]
        assert vn.tolist() == [8] * h and vf.tolist() == [0] * h
    cy, cyf, _, _ = model.v_taps(8, "left")
    assert cy.tolist() == [0, 1, 0, 1, 2, 3, 2, 3] and cyf.tolist() == [0, 1, 2, 3, 0, 1, 2, 3]
    assert model.v_taps(6, "left")[0][5] == 1 and model.v_taps(6, "left")[1][5] == 1          # h % 4 == 2: row 5 reads its field's last chroma row
    for h in (4, 6, 8, 10, 12, 22):                                                          # a row never reads the other field's chroma
        for chroma in model.CHROMAS:
            cy, cyf, vn, vf = model.v_taps(h, chroma)
            y = np.arange(h)
            assert ((cy & 1) == (y & 1)).all() and ((cyf & 1) == (y & 1)).all() and cy.max() < h // 2 and cyf.max() < h // 2
            assert ((vn + vf) == 8).all()
    for w in (1, 2, 5, 8):                                                                   # horizontal: the sited stage's, or the own sample
        for chroma in ("left", "center"):
            assert all(np.array_equal(a, b) for a, b in zip(model.h_taps(w, chroma), sited_model.h_taps(w, chroma)))
        cx, cxf, hn, hf = model.h_taps(w, "replicate")
        assert cx.tolist() == cxf.tolist() == [x >> 1 for x in range(w)] and hn.tolist() == [4] * w and hf.tolist() == [0] * w
    for chroma in model.CHROMAS:                                                             # D of single impulses: the weights sum to 32
        h, w = 10, 7
        total = np.zeros((h, w), dtype=np.int64)
        for r in range(h // 2):
            for c in range((w + 1) // 2):
                imp = np.zeros((h // 2, (w + 1) // 2), dtype=np.int64)
                imp[r, c] = 1
                total += model.interpolate(imp, h, w, chroma)
        assert (total == 32).all()
    for h in (0, 2, 5, 7):
        with pytest.raises(AssertionError):
            model.v_taps(h, "left")


# ---- ties to the replicating stages' models ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", model.LAYOUTS)
def test_literals_and_geometry_are_the_existing_families(layout):
    from pythoncrt_amd import field420
    assert model.MATRICES8 is unpack_model.MATRICES and model.MATRICES10 is deep_model.RGB_MATRICES
    for matrix, rng in model.CASES:
        m, off, top = model.tables(layout, matrix, rng)
        tm, toff = (tables.rgb_matrix10 if layout in model.DEEP else tables.rgb_matrix)(matrix, rng)
        assert np.array_equal(m.reshape(-1), tm) and tuple(toff) == tuple(off) and top == (1020 if layout in model.DEEP else 255)
    for h, w in ((4, 1), (6, 7), (16, 64), (38, 131), (1080, 1920)):
        want = (h * w + 2 * (h // 2) * ((w + 1) // 2)) * (2 if layout in model.DEEP else 1)
        assert field420.frame_bytes(h, w, layout) == model.frame_bytes(h, w, layout) == want
    assert list(field420.LAYOUTS) == list(model.LAYOUTS) and list(field420.LAYOUTS.values()) == list(range(4))
    assert list(field420.CHROMAS) == list(model.CHROMAS) and list(field420.CHROMAS.values()) == [0, 1, 2]
    with pytest.raises(ValueError):
        field420.frame_bytes(4, 4, "yuv422p")


@pytest.mark.parametrize("layout", model.LAYOUTS)
def test_replicate_is_the_weave_of_the_existing_stages_on_the_two_fields(layout):
    """h % 4 == 0, chroma "replicate": zero differing elements against the existing replicating model run on each field as an h/2 x w frame
    of its own, for every matrix and range — and the progressive model of the whole frame gives something else."""
    for matrix, rng in model.CASES:
        for h, w in ((4, 1), (4, 8), (8, 16), (12, 7), (16, 33)):
            for p in model.images(h, w, layout):
                got, exp = model.unpack(p, h, w, layout, "replicate", matrix, rng), model.weave_of_fields(p, h, w, layout, matrix, rng)
                assert got.dtype == exp.dtype and np.array_equal(_bits(got), _bits(exp)), (h, w, matrix, rng)
    p = model.images(16, 32, layout)[0]
    assert (_bits(model.unpack(p, 16, 32, layout)) != _bits(model.progressive(p, 16, 32, layout))).mean() > 0.2


@pytest.mark.parametrize("chroma", model.CHROMAS)
@pytest.mark.parametrize("layout", model.LAYOUTS)
def test_constant_chroma_gives_the_replicating_stage_s_bytes(layout, chroma):
    """Equal taps: floor((32 A + 2^20) / 2^21) = floor((A + 2^15) / 2^16), so constant chroma planes under random luma convert to the
    existing model's bytes, for all four matrices, h % 4 of 0 and 2."""
    rs = np.random.default_rng(5)
    top = 1024 if layout in model.DEEP else 256
    for matrix, rng in model.CASES:
        for h, w in ((4, 1), (6, 7), (8, 16), (18, 33)):
            for u0, v0 in ((0, top - 1), (top - 1, 0), (int(rs.integers(top)), int(rs.integers(top)))):
                y = rs.integers(0, top, (h, w))
                p = model.pack_planes(y, np.full((h // 2, (w + 1) // 2), u0), np.full((h // 2, (w + 1) // 2), v0), layout)
                got, exp = model.unpack(p, h, w, layout, chroma, matrix, rng), model.progressive(p, h, w, layout, "replicate", matrix, rng)
                assert got.dtype == exp.dtype and np.array_equal(_bits(got), _bits(exp)), (h, w, matrix, rng, u0, v0)
    a = np.arange(-3 * 2 ** 24, 3 * 2 ** 24, 4099, dtype=np.int64)
    assert np.array_equal((32 * a + 2 ** 20) >> 21, (a + 2 ** 15) >> 16)


def test_a_vertical_ramp_at_interlaced_siting_is_reproduced():
    """The sample of frame chroma row c is 8 x its true position in frame luma rows: 4 j + 0.5 for c = 2 j (top field: a quarter field row
    below luma row 4 j), 4 j + 2.5 for c = 2 j + 1 (bottom field: three quarters of a field row below luma row 4 j + 1).  Every row whose
    taps are unclamped then interpolates 8 y exactly: D = 32 * 8 y, the vertical blend in eighths being 8 * 8 y.  When one field's chroma
    then moves, the other field's rows stay on the line; under the progressive sited model they leave it."""
    h, w = 32, 8
    c = np.arange(h // 2)
    pos = np.where(c % 2 == 0, 4 * (c // 2) + 0.5, 4 * (c // 2) + 2.5)
    plane = np.tile((8 * pos).astype(np.int64)[:, None], (1, w // 2))
    assert plane[:4, 0].tolist() == [4, 20, 36, 52] and plane.max() < 256
    y = np.arange(h)
    for chroma in ("left", "center"):
        d = model.interpolate(plane, h, w, chroma)
        assert (d[4:28] == (256 * y[4:28])[:, None]).all(), chroma
        assert (d == d[:, :1]).all()
        assert not (d[:4] == (256 * y[:4])[:, None]).all() and not (d[28:] == (256 * y[28:])[:, None]).all()       # the clamped ends flatten
        # the positions 4 j + 0.5 and 4 j + 2.5 are 2 c + 0.5, the progressive siting's own: on a ramp that stands still the progressive
        # sited model lands on the same line, from rows of BOTH fields — what tells the two apart is motion (the field independence below)
        prog = 2 * sited_model.interpolate(plane, h, w, chroma, True)                                                 # 16ths -> 32nds
        assert (prog[4:28] == (256 * y[4:28])[:, None]).all()
        moved = plane.copy()
        moved[1::2] += 40                                                                                                # the bottom field, an instant later
        assert (model.interpolate(moved, h, w, chroma)[4:28:2] == (256 * y[4:28:2])[:, None]).all()                    # the top field's rows: untouched
        assert (2 * sited_model.interpolate(moved, h, w, chroma, True)[4:28:2] != (256 * y[4:28:2])[:, None]).all()
    rep = model.interpolate(plane, h, w, "replicate")
    assert (rep[:, 0] == 32 * plane[model.v_taps(h, "replicate")[0], 0]).all()


@pytest.mark.parametrize("layout", model.LAYOUTS)
def test_the_two_fields_are_independent(layout):
    """New chroma rows for ONE field leave every RGB row of the other field as it was, bit for bit, under all three chroma values; the
    progressive models change rows of the other field."""
    top = 1024 if layout in model.DEEP else 256
    rs = np.random.default_rng(9)
    for h, w in ((8, 6), (10, 16)):
        y, u, v = (rs.integers(0, top, s) for s in ((h, w), (h // 2, (w + 1) // 2), (h // 2, (w + 1) // 2)))
        for f in (0, 1):
            u2, v2 = u.copy(), v.copy()
            u2[f::2], v2[f::2] = (top - 1) - u[f::2], (top - 1) - v[f::2]
            a, b = model.pack_planes(y, u, v, layout), model.pack_planes(y, u2, v2, layout)
            for chroma in model.CHROMAS:
                ra, rb = _bits(model.unpack(a, h, w, layout, chroma)), _bits(model.unpack(b, h, w, layout, chroma))
                assert np.array_equal(ra[1 - f::2], rb[1 - f::2]) and not np.array_equal(ra[f::2], rb[f::2]), (h, w, f, chroma)
                pa, pb = _bits(model.progressive(a, h, w, layout, chroma)), _bits(model.progressive(b, h, w, layout, chroma))
                assert not np.array_equal(pa[1 - f::2], pb[1 - f::2]), (h, w, f, chroma)


# ---- the integer model against the float restatement -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("matrix,rng", model.CASES)
@pytest.mark.parametrize("layout", ("nv12", "yuv420p10le"))
def test_model_against_the_float_restatement(layout, matrix, rng):
    """The interpolation is exact in both (D / 32 is a dyadic fraction of 15 bits), so the two differ only by the rounding of the matrix:
    every entry is the float one rounded to 2^-16, at most 2^-17 off, times a centred sample of at most max_sample in magnitude, three
    entries to a row: the value in front of the floor moves by at most 3 * max_sample * 2^-17 (plus float64's own rounding, below 1e-9).
    The codes are therefore equal unless the float value lies that close to a half-integer, and then they differ by one."""
    bound = 3 * (1023 if layout in model.DEEP else 255) * 2.0 ** -17 + 1e-9
    for chroma in model.CHROMAS:
        for h, w in ((18, 33), (32, 64)):
            for p in model.images(h, w, layout)[:2]:
                got = model.codes(p, h, w, layout, chroma, matrix, rng)
                exp, raw = model.unpack_float(p, h, w, layout, chroma, matrix, rng)
                d = got - exp
                assert np.abs(d).max() <= 1
                dist = np.abs(raw - np.floor(raw) - 0.5)
                assert (dist[d != 0] <= bound).all(), float(dist[d != 0].max())


# ---- accumulators ----------------------------------------------------------------------------------------------------------------------------

def test_accumulator_bounds_of_all_eight_matrices():
    """8-bit: the header's rule holds for the four matrices, the largest sum bt709 limited range at about 1.75e9.  10-bit: no row of the
    limited-range matrices fits int32, neither whole nor split: the luma part alone passes 2^31 and so does the chroma part of a row.
    The header's rearrangement — S + floor(R / 32) in int32, then one shift by 16 — gives the int64 accumulator's code at every corner
    of the sample cube and on random samples, for the four matrices and for one on the admission rule's boundary; its rule holds for
    the four by a factor of more than 6."""
    worst8 = {}
    for key, m in model.MATRICES8.items():
        for row in m:
            worst = sum(abs(c) for c in row) * 255 * 32 + (1 << 20)
            assert worst < 2 ** 31, (key, row, worst)
            worst8[key] = max(worst8.get(key, 0), worst)
    assert max(worst8, key=worst8.get) == ("bt709", "tv") and 1.7e9 < worst8[("bt709", "tv")] < 1.8e9
    for key, m in model.MATRICES10.items():
        off = model.OFFSETS10[key[1]]
        span = [32 * max(o, 1023 - o) for o in off]
        whole = max(sum(abs(c) * s for c, s in zip(row, span)) + (1 << 20) for row in m)
        assert whole >= 2 ** 31, key
        if key[1] == "tv":
            assert max(abs(row[0]) * span[0] for row in m) >= 2 ** 31 and abs(m[0][0]) * span[0] > 2.3e9
            assert 2.1e9 < max(abs(row[1]) * span[1] + abs(row[2]) * span[2] for row in m) < 2.3e9
        assert max(sum(abs(c) for c in row) for row in m) * 1024 * 6 + 2 ** 15 < 2 ** 31
    s10 = (2 ** 31 - 2 ** 15 - 1) // 1024
    assert s10 * 1024 + 2 ** 15 < 2 ** 31 <= (s10 + 1) * 1024 + 2 ** 15 and s10 < 2 ** 22
    rs = np.random.default_rng(10)
    corners = np.array([(y, u, v) for y in (0, 1023) for u in (0, 32 * 1023, 31, 32 * 1023 - 31) for v in (0, 32 * 1023, 1, 32 * 1022 + 1)])
    samples = np.concatenate([corners, np.stack([rs.integers(0, 1024, 4000), rs.integers(0, 32 * 1023 + 1, 4000), rs.integers(0, 32 * 1023 + 1, 4000)], axis=1)])
    rows = [(row, model.OFFSETS10[key[1]]) for key, m in model.MATRICES10.items() for row in m]
    rows += [((s10 - 7, -3, 4), (64, 512, 512)), ((-5, s10 - 5, 0), (0, 0, 1023)), ((0, -(s10 // 2), -(s10 - s10 // 2)), (1023, 1023, 0))]
    for row, off in rows:
        y, du, dv = samples[:, 0], samples[:, 1], samples[:, 2]
        c, d, e = y - off[0], du - 32 * off[1], dv - 32 * off[2]
        acc = 32 * row[0] * c + row[1] * d + row[2] * e + 2 ** 20
        s_ = row[0] * c + row[1] * (d >> 5) + row[2] * (e >> 5)
        r_ = row[1] * (d & 31) + row[2] * (e & 31) + 2 ** 20
        for part in (s_, r_, s_ + (r_ >> 5)):
            assert np.abs(part).max() < 2 ** 31, (row, off)
        assert np.array_equal(acc >> 21, (s_ + (r_ >> 5)) >> 16), (row, off)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------

SEVEN = ("create", "destroy", "last_error", "frame_bytes", "run", "set_option", "last_plan")


def test_header_prototypes_are_the_bound_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_field420_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(_lib.FIELD420_SYMBOLS) == {f"crtfx_field420_{n}" for n in SEVEN}, set(protos) ^ set(_lib.FIELD420_SYMBOLS)
    assert _lib.FIELD420_SYMBOLS == _lib.stage_symbols("field420")
    for name, args in protos.items():
        assert len(args.split(",")) == len(_lib.FIELD420_SYMBOLS[name][1]), name
        assert _lib.FIELD420_SYMBOLS[name] == _lib.UNPACK_SYMBOLS[name.replace("crtfx_field420_", "crtfx_unpack_")], name
    enum = re.search(r"enum crtfx_field420_layout\s*\{(.*?)\}", hdr, re.S).group(1)
    assert [(n, int(v)) for n, v in re.findall(r"CRTFX_FIELD420_(\w+)\s*=\s*(\d+)", enum)] == [(l.upper(), i) for i, l in enumerate(model.LAYOUTS)]
    assert re.search(r"CRTFX_FIELD420_REPLICATE\s*=\s*0\s*,\s*CRTFX_FIELD420_LEFT\s*=\s*1\s*,\s*CRTFX_FIELD420_CENTER\s*=\s*2", hdr)
    assert re.search(r"CRTFX_FIELD420_OPT_FORCE_GENERAL\s*=\s*1\s*,\s*CRTFX_FIELD420_OPT_CHROMA\s*=\s*2", hdr)
    assert (_lib.FIELD420_REPLICATE, _lib.FIELD420_LEFT, _lib.FIELD420_CENTER, _lib.FIELD420_OPT_FORCE_GENERAL, _lib.FIELD420_OPT_CHROMA) == (0, 1, 2, 1, 2)
    assert [getattr(_lib, "FIELD420_" + l.upper()) for l in model.LAYOUTS] == list(range(4))
    assert all(os.path.basename(f) in {os.path.basename(s) for s in _lib.SOURCES} for f in ("crtfx_field420.hip", "crtfx_field420.h"))
    assert "crtfx_field420" in _lib.STAGE_UNITS
    lib = _lib.load()
    for name in _lib.FIELD420_SYMBOLS:
        assert getattr(lib, name).argtypes == _lib.FIELD420_SYMBOLS[name][1]
    import pythoncrt_amd as pc
    assert pc.UnpackField420.__name__ in pc.__all__ and issubclass(pc.UnpackField420, _stage.SourcePlan)


def _create(lib, layout=_lib.FIELD420_NV12, h=12, w=20, pix_fmt=None, device=0, m=None, off=None, null=False, null_off=False):
    deep = layout in (_lib.FIELD420_YUV420P10LE, _lib.FIELD420_P010LE)
    tm, toff = (tables.rgb_matrix10 if deep else tables.rgb_matrix)("bt601", "tv")
    m = tm if m is None else np.ascontiguousarray(m, dtype=np.int32)
    off = toff if off is None else np.ascontiguousarray(off, dtype=np.int32)
    pix_fmt = (_lib.PIX_F16 if deep else _lib.PIX_U8) if pix_fmt is None else pix_fmt
    plan = ctypes.c_void_p(1)
    rc = lib.crtfx_field420_create(device, h, w, pix_fmt, layout, None if null else tables.ptr(m), None if null_off else tables.ptr(off), ctypes.byref(plan))
    return rc, plan, (lib.crtfx_field420_last_error(None) or b"").decode()


def test_create_refuses_bad_arguments_before_it_touches_a_device():
    """The argument checks come first, so they hold on any machine: an odd height, one below 4, the other pixel format (UNSUPPORTED), an
    unknown one, sizes, layouts, null tables, offsets and an 8-bit matrix one step past the header's admission rule (INVALID); each leaves
    *out_plan NULL and a message.  A matrix on either rule's boundary is admitted."""
    lib = _lib.load()
    good8, good10 = tables.rgb_matrix("bt601", "tv")[0], tables.rgb_matrix10("bt601", "tv")[0]
    s8 = (2 ** 31 - 2 ** 20 - 1) // 8160                               # s * 255 * 32 + 2^20 < 2^31
    assert s8 * 8160 + 2 ** 20 < 2 ** 31 <= (s8 + 1) * 8160 + 2 ** 20
    s10 = (2 ** 31 - 2 ** 15 - 1) // 1024                              # s * 1024 + 2^15 < 2^31
    assert s10 * 1024 + 2 ** 15 < 2 ** 31 <= (s10 + 1) * 1024 + 2 ** 15
    fits8, over8, split8, fits10, over10, split10 = good8.copy(), good8.copy(), good8.copy(), good10.copy(), good10.copy(), good10.copy()
    fits8[0:3] = (s8, 0, 0)
    over8[0:3] = (s8 + 1, 0, 0)
    split8[3:6] = (s8 - 9, -5, 5)                                      # the rule sums magnitudes: one past in all
    fits10[0:3] = (s10 - 7, -3, 4)
    over10[6:9] = (0, s10 + 1, 0)
    split10[3:6] = (-(s10 - 9), -5, 5)
    cases = [(dict(h=11), _lib.E_INVALID, "odd"), (dict(h=7, layout=_lib.FIELD420_P010LE), _lib.E_INVALID, "odd"), (dict(h=1), _lib.E_INVALID, "odd"),
             (dict(h=2), _lib.E_INVALID, "below 4"), (dict(h=0), _lib.E_INVALID, "below 4"), (dict(h=-2), _lib.E_INVALID, "below 4"),
             (dict(pix_fmt=_lib.PIX_F16), _lib.E_UNSUPPORTED, "uint8"), (dict(layout=_lib.FIELD420_YUV420P, pix_fmt=_lib.PIX_F16), _lib.E_UNSUPPORTED, "uint8"),
             (dict(layout=_lib.FIELD420_P010LE, pix_fmt=_lib.PIX_U8), _lib.E_UNSUPPORTED, "half"),
             (dict(layout=_lib.FIELD420_YUV420P10LE, pix_fmt=_lib.PIX_U8), _lib.E_UNSUPPORTED, "half"),
             (dict(pix_fmt=7), _lib.E_INVALID, "pixel format"), (dict(layout=_lib.FIELD420_P010LE, pix_fmt=-1), _lib.E_INVALID, "pixel format"),
             (dict(w=0), _lib.E_INVALID, "size"), (dict(w=32768), _lib.E_INVALID, "size"), (dict(h=32768), _lib.E_INVALID, "size"),
             (dict(layout=4), _lib.E_INVALID, "layout"), (dict(layout=-1), _lib.E_INVALID, "layout"), (dict(layout=4, pix_fmt=_lib.PIX_F16), _lib.E_INVALID, "layout"),
             (dict(null=True), _lib.E_INVALID, "null"), (dict(null_off=True), _lib.E_INVALID, "null"),
             (dict(off=(16, 256, 128)), _lib.E_INVALID, "offset"), (dict(off=(-1, 128, 128)), _lib.E_INVALID, "offset"),
             (dict(layout=_lib.FIELD420_P010LE, off=(64, 512, 1024)), _lib.E_INVALID, "offset"),
             (dict(m=over8), _lib.E_INVALID, "accumulator"), (dict(m=split8), _lib.E_INVALID, "accumulator"),
             (dict(layout=_lib.FIELD420_YUV420P, m=over8), _lib.E_INVALID, "accumulator"),
             (dict(layout=_lib.FIELD420_P010LE, m=over10), _lib.E_INVALID, "accumulator"), (dict(layout=_lib.FIELD420_YUV420P10LE, m=split10), _lib.E_INVALID, "accumulator")]
    for kw, code, word in cases:
        rc, plan, msg = _create(lib, **kw)
        assert rc == code and not plan.value and word in msg, (kw, rc, plan.value, msg)
    ok = [dict(m=fits8), dict(layout=_lib.FIELD420_P010LE, m=fits10), dict(layout=_lib.FIELD420_YUV420P10LE, m=fits10), dict(h=32766, w=32767), dict(h=4, w=1),
          dict(layout=_lib.FIELD420_P010LE, off=(64, 512, 1023))]
    ok += [dict(layout=i) for i in range(4)]
    # all eight matrices of tables are admitted
    ok += [dict(layout=_lib.FIELD420_NV12, m=tables.rgb_matrix(*c)[0], off=tables.rgb_matrix(*c)[1]) for c in model.CASES]
    ok += [dict(layout=_lib.FIELD420_P010LE, m=tables.rgb_matrix10(*c)[0], off=tables.rgb_matrix10(*c)[1]) for c in model.CASES]
    for kw in ok:
        rc, plan, msg = _create(lib, **kw)
        assert rc in (_lib.OK, _lib.E_HIP), (kw, rc, msg)             # no device here: E_HIP; with one: a plan
        if rc == _lib.OK:
            assert lib.crtfx_field420_set_option(plan, 2, 3) == _lib.E_INVALID and b"CHROMA" in lib.crtfx_field420_last_error(plan)
            assert lib.crtfx_field420_set_option(plan, 2, -1) == _lib.E_INVALID and lib.crtfx_field420_set_option(plan, 3, 0) == _lib.E_INVALID
            assert b"option 3" in lib.crtfx_field420_last_error(plan)
            assert lib.crtfx_field420_set_option(plan, 1, 2) == _lib.E_INVALID and b"FORCE_GENERAL" in lib.crtfx_field420_last_error(plan)
            assert lib.crtfx_field420_destroy(plan) == _lib.OK
    assert lib.crtfx_field420_create(0, 12, 20, _lib.PIX_U8, _lib.FIELD420_NV12, tables.ptr(good8), tables.ptr(tables.rgb_matrix("bt601", "tv")[1]), None) == _lib.E_INVALID
    assert b"out_plan" in lib.crtfx_field420_last_error(None)
    assert lib.crtfx_field420_destroy(None) == _lib.OK and lib.crtfx_field420_set_option(None, 1, 1) == _lib.E_INVALID
    assert lib.crtfx_field420_set_option(None, 2, 1) == _lib.E_INVALID
    assert lib.crtfx_field420_run(None, None, 0, None, 0, 1, None) == _lib.E_INVALID and lib.crtfx_field420_frame_bytes(None) == 0
    assert lib.crtfx_field420_last_plan(None, ctypes.create_string_buffer(8), 8) == _lib.E_INVALID


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
    from pythoncrt_amd import UnpackField420
    with pytest.raises(ValueError) as e:
        UnpackField420("cuda", (8, 8), "nv12", chroma="top-left")
    assert "chroma" in str(e.value)
    with pytest.raises(ValueError):
        UnpackField420("cpu", (8, 8), "nv12")


# ---- refusals of process_frames, probe_frames and the two CLIs ----------------------------------------------------------------------------------

ROWS_TEXT = "in_chroma_rows must be 'progressive' or 'interlaced', got {!r}"
FORMAT_TEXT = "in_chroma_rows='interlaced' with in_pix_fmt={!r}: only a 4:2:0 input has chroma rows that two fields share " + FOUR
HEIGHT_TEXT = "in_chroma_rows='interlaced': a source frame of {} row(s) has no two fields of whole chroma rows (an even height of at least 4)"
FORMAT_FLAGS = "--in-chroma-rows interlaced with --in-pix-fmt {}: only a 4:2:0 input has chroma rows that two fields share " + FOUR
HEIGHT_FLAGS = "--in-chroma-rows interlaced with --height {0}: a frame of {0} row(s) has no two fields of whole chroma rows (an even height of at least 4)"
# (keywords, (out_h, out_w), the text)
KEYWORD_CASES = [
    (dict(in_chroma_rows="field"), (36, 64), ROWS_TEXT.format("field")),
    (dict(in_chroma_rows=None, in_pix_fmt="nv12"), (36, 64), ROWS_TEXT.format(None)),
    (dict(in_chroma_rows=["interlaced"], in_pix_fmt="nv12"), (36, 64), ROWS_TEXT.format(["interlaced"])),
    (dict(in_chroma_rows="interlaced"), (36, 64), FORMAT_TEXT.format("rgb24")),
    (dict(in_chroma_rows="interlaced", in_pix_fmt="yuv422p"), (36, 64), FORMAT_TEXT.format("yuv422p")),
    (dict(in_chroma_rows="interlaced", in_pix_fmt="uyvy422", in_chroma="left"), (36, 64), FORMAT_TEXT.format("uyvy422")),
    (dict(in_chroma_rows="interlaced", in_pix_fmt="nv12"), (37, 64), HEIGHT_TEXT.format(37)),
    (dict(in_chroma_rows="interlaced", in_pix_fmt="yuv420p", in_size=(2, 64)), (36, 64), HEIGHT_TEXT.format(2)),
    (dict(in_chroma_rows="interlaced", in_pix_fmt="yuv420p", in_size=(21, 64), in_chroma="center"), (36, 64), HEIGHT_TEXT.format(21)),
]


def _never():
    raise AssertionError("a frame was read")
    yield


@pytest.fixture
def no_device(monkeypatch):
    import torch

    def asked():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", asked)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("CRTFX_FORCE_DIST", raising=False)


def test_process_frames_and_probe_frames_refuse_before_they_touch_a_device(no_device):
    import pythoncrt_amd as pc
    for kw, (oh, ow), text in KEYWORD_CASES:
        with pytest.raises(ValueError) as e:
            pc.process_frames(_never(), lambda a: (_ for _ in ()).throw(AssertionError("written")), ow, oh, 30.0, 1, **kw)
        assert str(e.value) == text, (kw, str(e.value))
        with pytest.raises(ValueError) as e:
            pc.probe_frames(_never(), ow, oh, **kw)
        assert str(e.value) == text, (kw, str(e.value))
    for fmt in ("yuv444p10le", "gbrp10le", "x2rgb10le"):
        with pytest.raises(ValueError) as e:
            pc.process_frames(_never(), lambda a: None, 64, 36, 30.0, 1, in_chroma_rows="interlaced", in_pix_fmt=fmt, out_pix_fmt=fmt)
        assert str(e.value) == FORMAT_TEXT.format(fmt)
    # the rules in front of it keep their place: RULES is walked first
    for kw, word in ((dict(in_chroma_rows="interlaced", in_pix_fmt="p010le"), "one end"), (dict(in_chroma_rows="interlaced", in_pix_fmt="nv12", resize_on="host"), "host"),
                     (dict(in_chroma_rows="interlaced", in_chroma="left"), "in_chroma=")):
        with pytest.raises(ValueError) as e:
            pc.process_frames(_never(), lambda a: None, 64, 36, 30.0, 1, **kw)
        assert word in str(e.value), (kw, str(e.value))


def test_both_clis_have_the_flag_and_its_refusals(no_device, monkeypatch, tmp_path, capsys):
    from pythoncrt_amd import cli, probe
    parser = cli.add_input_flags(cli.add_output_flags(cli.build_parser()))
    assert parser.parse_args(["--input", "x"]).in_chroma_rows == "progressive"
    assert probe.build_parser().parse_args(["--input", "x", "--width", "8", "--height", "8"]).in_chroma_rows == "progressive"
    for p, base in ((parser, ["--input", "x"]), (probe.build_parser(), ["--input", "x", "--width", "8", "--height", "8"])):
        for v in ("progressive", "interlaced"):
            assert p.parse_args(base + ["--in-chroma-rows", v]).in_chroma_rows == v
        with pytest.raises(SystemExit) as e:
            p.parse_args(base + ["--in-chroma-rows", "field"])
        assert e.value.code == 2
    src, out = tmp_path / "in.raw", tmp_path / "out.raw"
    src.write_bytes(bytes(8 * 8 * 6))

    def argv(h, *extra):
        return ["--input", str(src), "--width", "8", "--height", str(h), "--in-chroma-rows", "interlaced", *extra]
    cases = [(argv(8), FORMAT_FLAGS.format("rgb24")), (argv(8, "--in-pix-fmt", "yuyv422"), FORMAT_FLAGS.format("yuyv422")),
             (argv(7, "--in-pix-fmt", "nv12"), HEIGHT_FLAGS.format(7)), (argv(2, "--in-pix-fmt", "yuv420p", "--in-chroma", "left"), HEIGHT_FLAGS.format(2))]
    for args, text in cases:
        with pytest.raises(SystemExit) as e:
            cli.main(args + ["--output", str(out)])
        assert e.value.code == text and getattr(e.value.__cause__, "rule", "").startswith("in_chroma_rows") and not out.exists(), (args, e.value.code)
        with pytest.raises(SystemExit) as e:
            probe.main(args)
        assert e.value.code == text, (args, e.value.code)
    with pytest.raises(SystemExit) as e:                            # 10-bit: the CLI needs both ends, the probe has one
        cli.main(argv(7, "--in-pix-fmt", "p010le", "--out-pix-fmt", "p010le", "--output", str(out)))
    assert e.value.code == HEIGHT_FLAGS.format(7)
    with pytest.raises(SystemExit) as e:
        probe.main(argv(6, "--in-pix-fmt", "gbrp10le"))
    assert e.value.code == FORMAT_FLAGS.format("gbrp10le")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:                            # early: in front of the sharded CLI's branch
        cli.main(argv(8) + ["--output", str(out)])
    assert e.value.code == FORMAT_FLAGS.format("rgb24") and not out.exists()
    with pytest.raises(SystemExit) as e:                            # the height is not known there before the branch asks for it
        cli.main(["--input", str(src), "--width", "8", "--in-chroma-rows", "interlaced", "--in-pix-fmt", "nv12", "--output", str(out)])
    assert "--in-chroma-rows" not in str(e.value.code) and not out.exists()
    capsys.readouterr()


def test_field_rules_fire_on_the_surfaces_they_speak_on():
    """FIELD_RULES is a table of its own behind RULES (whose recorded cases tests/test_chain_options.py holds): three entries, all in front
    of the sharded branch; the membership check speaks to the keywords only, the other two to both surfaces."""
    from pythoncrt_amd import options
    assert [r.name for r in options.FIELD_RULES] == ["in_chroma_rows", "in_chroma_rows_format", "in_chroma_rows_height"]
    assert all(type(r) is options.Rule and r.early for r in options.FIELD_RULES)
    assert [(r.keywords is not None, r.flags is not None) for r in options.FIELD_RULES] == [(True, False), (True, True), (True, True)]
    assert not {r.name for r in options.FIELD_RULES} & {r.name for r in options.RULES}

    def raw(hw=(36, 64), **kw):
        return options.Raw(render_hw=hw, **{n: kw.get(n, d) for n, d in _DEFAULTS.items()})
    fired = set()
    cases = [("in_chroma_rows", dict(in_chroma_rows="both"), ("keywords",)), ("in_chroma_rows_format", dict(in_chroma_rows="interlaced"), ("keywords", "flags")),
             ("in_chroma_rows_height", dict(in_chroma_rows="interlaced", in_pix_fmt="nv12", in_size=(6, 7 * 3)), ()),
             ("in_chroma_rows_height", dict(in_chroma_rows="interlaced", in_pix_fmt="nv12", in_size=(9, 16)), ("keywords", "flags"))]
    for name, kw, surfaces in cases:
        for surface in ("keywords", "flags"):
            for early in (None, True):
                try:
                    options.refuse(raw(**kw), surface, early)
                    got = None
                except options.OptionError as e:
                    got = e.rule
                assert got == (name if surface in surfaces else None), (name, kw, surface, early, got)
            options.refuse(raw(**kw), surface, False)                 # behind the branch none of the three is walked
            fired |= {(name, surface)} if surface in surfaces else set()
    assert fired == {(r.name, s) for r in options.FIELD_RULES for s in ("keywords", "flags") if getattr(r, s) is not None}
    v = raw(hw=(None, 64), in_chroma_rows="interlaced", in_pix_fmt="nv12")
    v.in_size = (None, 64)
    options.refuse(v, "flags", True)                                  # a height not given yet is not checked
    assert raw().in_chroma_rows == "progressive" and options.Raw(render_hw=(8, 8)).in_chroma_rows == "progressive"


# the keywords of process_frames that a Raw holds
_RAW = ("resize_on", "out_pix_fmt", "out_matrix", "out_range", "in_pix_fmt", "in_matrix", "in_range", "in_size", "in_chroma", "out_chroma",
        "deliver_size", "in_filter", "deliver_filter", "in_crop", "deliver_fit", "deliver_pad_color", "chain_pix", "dither", "deinterlace",
        "field_order", "deinterlace_fields", "in_lut", "deliver_lut", "deliver_interlace", "deliver_lowpass", "in_signal", "signal_chroma",
        "signal_crawl", "in_chroma_rows")


# ---- the plans the ends build -------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def built(monkeypatch):
    """tests/test_chain_ends.py's recorders over every class a SourceEnd may construct: (class, positional arguments, keywords)."""
    from pythoncrt_amd import adeint, canvas, deint, depth, field420, ingest, lut3d, resample, resize16, signal as signal_mod
    from tests.test_chain_ends import STAGES
    log = []
    others = [ingest.IngestResize, resize16.ResizeHalf, resample.Resample, signal_mod.Signal, deint.Deinterlace, adeint.AdaptiveDeinterlace, canvas.Canvas,
              depth.Widen, depth.Narrow, lut3d.Lut3D]
    for cls in STAGES + [field420.UnpackField420] + others:
        def init(self, *args, _cls=cls, **kw):
            log.append((_cls, args, kw))
            if issubclass(_cls, _stage.StagePlan):
                self.frame_bytes = _cls._frame_bytes(args[1][0], args[1][1], kw["layout"])
        monkeypatch.setattr(cls, "__init__", init)
    return log


def test_source_plan_and_the_source_end(built, monkeypatch):
    import torch
    from pythoncrt_amd import deint, ends, field420, formats, ingest, options, sited, unpack
    # formats.source_plan: the seventh parameter
    for fmt in model.LAYOUTS:
        for chroma in model.CHROMAS:
            del built[:]
            plan = formats.source_plan("dev", (8, 10), fmt, "bt709", "pc", chroma, "interlaced")
            assert type(plan) is field420.UnpackField420
            assert built == [(field420.UnpackField420, ("dev", (8, 10)), {"layout": fmt, "matrix": "bt709", "range": "pc", "chroma": chroma})]
            del built[:]
            assert type(formats.source_plan("dev", (8, 10), fmt, "bt709", "pc", chroma, rows="progressive")) is not field420.UnpackField420
            assert type(formats.source_plan("dev", (8, 10), fmt, "bt709", "pc", chroma)) is type(formats.source_plan("dev", (8, 10), fmt, "bt709", "pc", chroma, "progressive"))
    assert formats.source_plan("dev", (8, 10), "rgb24", "bt601", "tv", "replicate", "interlaced") is None
    # SourceEnd: with the default, source_plan is called with today's six positional arguments and nothing more
    calls = []
    real = formats.source_plan
    monkeypatch.setattr(formats, "source_plan", lambda *a, **kw: calls.append((a, kw)) or real(*a, **kw))
    del built[:]
    end = ends.SourceEnd("dev", (16, 20), "nv12", "bt601", "tv", "left", (8, 10), "bilinear", None, torch.uint8, deinterlace=("linear", "tff", "both"))
    assert calls == [(("dev", (8, 10), "nv12", "bt601", "tv", "left"), {})]
    assert [b[0] for b in built] == [sited.UnpackSited, deint.Deinterlace, ingest.IngestResize] and end.ratio == 2
    del calls[:], built[:]
    end = ends.SourceEnd("dev", (16, 20), "nv12", "bt601", "tv", "left", (8, 10), "bilinear", None, torch.uint8, deinterlace=("linear", "tff", "both"),
                         chroma_rows="interlaced")
    assert calls == [(("dev", (8, 10), "nv12", "bt601", "tv", "left", "interlaced"), {})]
    assert [b[0] for b in built] == [field420.UnpackField420, deint.Deinterlace, ingest.IngestResize]
    assert built[0] == (field420.UnpackField420, ("dev", (8, 10)), {"layout": "nv12", "matrix": "bt601", "range": "tv", "chroma": "left"})
    assert type(end.plan) is field420.UnpackField420 and end.frame_bytes == 8 * 10 + 2 * 4 * 5 and end.stages[0] == (end.plan, (8, 10))
    del calls[:], built[:]
    ends.SourceEnd("dev", (8, 10), "yuv420p", "bt601", "tv", "replicate", (8, 10), "bilinear", chroma_rows="progressive")
    assert calls == [(("dev", (8, 10), "yuv420p", "bt601", "tv", "replicate"), {})] and [b[0] for b in built] == [unpack.UnpackYuv]
    # ChainOptions: the keyword is passed on only where it is not the default
    seen = []
    monkeypatch.setattr(ends, "SourceEnd", lambda *a, **kw: seen.append((a, kw)))

    def spec(**kw):
        v = options.Raw(render_hw=(8, 10), **{n: kw.get(n, d) for n, d in _DEFAULTS.items()})
        return options.ChainOptions.build(v, "keywords")
    a, b = spec(in_pix_fmt="nv12"), spec(in_pix_fmt="nv12", in_chroma_rows="interlaced", in_chroma="center")
    assert a.in_chroma_rows == "progressive" and type(a) is options.ChainOptions and b.in_chroma_rows == "interlaced" and isinstance(b, options.ChainOptions)
    assert a != b and not a.direct and not b.direct
    a.source_end("dev", (8, 10), torch.uint8)
    b.source_end("dev", (8, 10), torch.uint8)
    assert "chroma_rows" not in seen[0][1] and seen[1][1]["chroma_rows"] == "interlaced" and seen[1][0][5] == "center"
    assert {k: v for k, v in seen[1][1].items() if k != "chroma_rows"} == seen[0][1]


def _defaults():
    """Each of them at the default of process_frames' signature."""
    import inspect
    import pythoncrt_amd as pc
    sig = inspect.signature(pc.process_frames).parameters
    return {n: sig[n].default for n in _RAW}


_DEFAULTS = _defaults()


# ---- the kernel builds ----------------------------------------------------------------------------------------------------------------------------

def test_the_eight_kernel_builds_and_their_registers():
    """Exactly eight builds (four layouts x two paths) in crtfx_field420_impl, read from the library's code objects
    (tools/kernel_resources.py): no spills, no scratch, no LDS, no AGPRs, at most 128 registers — and the VGPR counts the header states."""
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n: v for n, v in res.items() if n.startswith("crtfx_field420_impl::")}
    assert set(found) == {f"crtfx_field420_impl::k_unpack_field420<{l}, {p}>" for l in range(4) for p in (0, 1)}, sorted(found)
    text = open(HEADER).read()
    stated = {name: (int(v), int(g)) for name, v, g in re.findall(r"(\w+) (\d+) / (\d+)", text[text.index("Registers (gfx950"):text.index("no AGPRs")])}
    assert list(stated) == list(model.LAYOUTS), stated
    for name, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == 0 and v["agpr_count"] == 0 and v["vgpr_count"] + v["agpr_count"] <= 128, (name, v)
        layout, path = map(int, re.search(r"<(\d), (\d)>", name).groups())
        assert v["vgpr_count"] == stated[model.LAYOUTS[layout]][1 - path], (name, v["vgpr_count"], stated)
