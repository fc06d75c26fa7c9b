"""The sited egress stage without a GPU: the identity that ties tests/egress_sited_model.py with the "center" weights to the three box
models, the index tables written out, a linear ramp, the integer model against its float64 restatement, the accumulator bounds of
include/crtfx_egress_sited.h, a round trip through the sited source model, the C-ABI bound symbol for symbol and failing cleanly without a
device, the refusals of the class, process_frames and the CLI, and the fourteen kernel builds' registers."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pythoncrt_amd import _lib, tables  # noqa: E402
from tests import deep_model, sited_model, unpack_model, yuv422_model, yuv_model  # noqa: E402
from tests import egress_sited_model as model  # noqa: E402

HEADER = os.path.join(ROOT, "include", "crtfx_egress_sited.h")
SIZES = [(1, 1), (2, 2), (3, 5), (5, 3), (4, 8), (6, 24), (5, 520), (37, 131)]


# ---- ties to the box stages' models ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", model.LAYOUTS)
def test_literals_and_geometry_are_the_existing_families(layout):
    assert model.MATRICES8 is yuv_model.MATRICES and model.MATRICES10 is deep_model.YUV_MATRICES
    from pythoncrt_amd import sited
    for matrix, rng in model.CASES:
        m, off, top = model.tables(layout, matrix, rng)
        tm, toff = (tables.yuv_matrix10 if layout in model.DEEP else tables.yuv_matrix)(matrix, rng)
        assert np.array_equal(m.reshape(-1), tm) and tuple(toff) == tuple(off) and top == (1023 if layout in model.DEEP else 255)
    for h, w in SIZES + [(1080, 1920)]:
        assert sited.frame_bytes(h, w, layout) == model.frame_bytes(h, w, layout) == sited_model.frame_bytes(h, w, layout)
    assert list(sited.LAYOUTS) == list(model.LAYOUTS) and model.LAYOUTS == sited_model.LAYOUTS


@pytest.mark.parametrize("layout", model.LAYOUTS)
def test_center_is_the_box_stage_byte_for_byte(layout):
    """(wl, w0, wr) = (0, 2, 2): S is twice the box sum and the shift has one more bit, so every byte is the box model's — for every input,
    here the three test images of the layout's family at every size of the GPU tests, and all four matrices at two of them."""
    assert model.WEIGHTS == {"left": (1, 2, 1), "center": (0, 2, 2)}
    for h, w in SIZES:
        for i, img in enumerate(model.images(h, w, layout)):
            for matrix, rng in (model.CASES if (h, w) in ((3, 5), (6, 24)) else [("bt601", "tv")]):
                got, exp = model.pack(img, layout, "center", matrix, rng), model.box(img, layout, matrix, rng)
                assert got.dtype == exp.dtype == np.uint8 and np.array_equal(got, exp), (h, w, i, matrix, rng)
    # ... and the sum itself
    p = np.random.default_rng(3).integers(0, 256, (5, 7, 3))
    assert np.array_equal(model.filter_sum(p, "nv12", "center"), 2 * yuv_model.box_sum(p))
    assert np.array_equal(model.filter_sum(p, "uyvy422", "center"), 2 * yuv422_model.pair_sum(p))
    assert np.array_equal(model.filter_sum(p, "p010le", "center"), 2 * deep_model.box_sum(p))


@pytest.mark.parametrize("layout", model.LAYOUTS)
def test_left_differs_from_center_on_a_random_frame(layout):
    """The weights are live: on a seeded random frame at least half of the chroma samples of "left" differ from "center"."""
    for h, w in ((6, 16), (5, 7), (36, 64)):
        rs = np.random.default_rng(100 * h + w)
        if layout in model.DEEP:
            img = (rs.integers(0, 1021, (h, w, 3)) / 4.0).astype(np.float16)
        else:
            img = rs.integers(0, 256, (h, w, 3), dtype=np.uint8)
        left = model.samples(model.pack(img, layout, "left"), h, w, layout)
        center = model.samples(model.pack(img, layout, "center"), h, w, layout)
        assert np.array_equal(left[0], center[0])                                   # Y is the box stage's, unchanged
        differ = np.concatenate([(left[i] != center[i]).reshape(-1) for i in (1, 2)])
        assert differ.mean() >= 0.5, (layout, h, w, float(differ.mean()))


# ---- the index tables, written out ------------------------------------------------------------------------------------------------------------

X_TAPS = {   # w: per chroma column (xl, x0, xr)
    1: [(0, 0, 0)],
    2: [(0, 0, 1)],
    5: [(0, 0, 1), (1, 2, 3), (3, 4, 4)],
    8: [(0, 0, 1), (1, 2, 3), (3, 4, 5), (5, 6, 7)],
}
Y_TAPS = {   # h: per chroma row (y0, y1), 4:2:0
    1: [(0, 0)],
    3: [(0, 1), (2, 2)],
    4: [(0, 1), (2, 3)],
}


def test_index_tables():
    for w, want in X_TAPS.items():
        t = model.x_taps(w)
        assert [tuple(int(a[cx]) for a in t) for cx in range((w + 1) // 2)] == want, w
    for h, want in Y_TAPS.items():
        t = model.y_taps(h, True)
        assert [tuple(int(a[cy]) for a in t) for cy in range((h + 1) // 2)] == want, h
        assert [tuple(int(a[y]) for a in model.y_taps(h, False)) for y in range(h)] == [(y, y) for y in range(h)]
    # S of single impulses: every sample's weights sum to 8 (4:2:0) or 4 (4:2:2) and land where the tables say
    for siting in model.SITINGS:
        for layout, total in (("nv12", 8), ("uyvy422", 4)):
            h, w = 5, 7
            acc = np.zeros(model.filter_sum(np.zeros((h, w, 3), dtype=np.int64), layout, siting).shape, dtype=np.int64)
            for y in range(h):
                for x in range(w):
                    imp = np.zeros((h, w, 3), dtype=np.int64)
                    imp[y, x] = 1
                    acc += model.filter_sum(imp, layout, siting)
            assert (acc == total).all(), (siting, layout)
    imp = np.zeros((1, 8, 3), dtype=np.int64)
    imp[0, 3] = 1                                                                   # an odd column feeds both neighbours with "left", one with "center"
    assert model.filter_sum(imp, "yuv422p", "left")[0, :, 0].tolist() == [0, 1, 1, 0]
    assert model.filter_sum(imp, "yuv422p", "center")[0, :, 0].tolist() == [0, 2, 0, 0]


@pytest.mark.parametrize("layout", ("nv12", "yuv422p", "p010le"))
def test_a_linear_ramp_gives_the_conversion_of_column_2cx(layout):
    """Channels linear in x (constant in y): [1 2 1] / 4 reproduces a linear function at its centre, so at interior columns S = 8 p[2 cx]
    (4:2:0) or 4 p[2 cx] (4:2:2) and the 19- / 18-bit shift is the Y-style 16-bit formula of the pixel at column 2 cx:
    (m . p + (off << 16) + (1 << 15)) >> 16.  With "center" the sample sits half a pixel to the right and it is not."""
    h, w = 4, 40
    x = np.arange(w, dtype=np.int64)
    scale = 4 if layout in model.DEEP else 1
    p = np.broadcast_to(np.stack([20 + 5 * x, 230 - 4 * x, 30 + 3 * x], axis=-1) * scale, (h, w, 3)).copy()
    m, off, top = model.tables(layout)
    direct = [np.clip((p[:, 0::2] @ m[k] + (off[k] << 16) + (1 << 15)) >> 16, 0, top) for k in (1, 2)]
    rows = model.y_taps(h, layout in model.V420)[0]
    _, u, v = model.convert_codes(p, layout, "left")
    inner = slice(1, w // 2)                                                       # cx >= 1: xl = 2 cx - 1 is a column of its own; xr = 2 cx + 1 < w always here
    assert np.array_equal(u[:, inner], direct[0][rows][:, inner]) and np.array_equal(v[:, inner], direct[1][rows][:, inner])
    assert not np.array_equal(u[:, 0], direct[0][rows][:, 0]) or not np.array_equal(v[:, 0], direct[1][rows][:, 0])      # the clamped tap flattens the start
    _, uc, vc = model.convert_codes(p, layout, "center")
    assert (uc[:, inner] != direct[0][rows][:, inner]).mean() > 0.25 and (vc[:, inner] != direct[1][rows][:, inner]).mean() > 0.25


# ---- the integer model against the float restatement -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("matrix,rng", model.CASES)
@pytest.mark.parametrize("layout", ("nv12", "uyvy422", "p010le"))
def test_model_against_the_float_restatement(layout, matrix, rng):
    """Random frames: the samples are the float64 ones except where the float value lies within 3 * max_sample * 2^-16 of a half-integer
    (tests/test_sited_tables.py's bound), and there they differ by one.  Derived here from the rounding of the integer matrix: the entries
    of a row differ from 65536 x the float ones by e0, e1, e2 (two rounded, the G entry adjusted), the filtered value of a channel is at
    most the largest per-pixel code (its weights are positive and sum to one), so the sums differ by at most (|e0| + |e1| + |e2|) * 2^-16
    * max code — and |e0| + |e1| + |e2| <= 3 for every row of all eight matrices, asserted below.  The filter itself is exact in both."""
    top_code = 1020 if layout in model.DEEP else 255
    bound = 3 * (1023 if layout in model.DEEP else 255) * 2.0 ** -16
    m, _, _ = model.tables(layout, matrix, rng)
    err = np.abs(m - 65536.0 * model.float_matrix(layout, matrix, rng)).sum(axis=1)
    assert (err <= 3.0).all() and err.max() * top_code * 2.0 ** -16 <= bound, err
    for siting in model.SITINGS:
        for h, w in ((17, 33), (32, 64)):
            for img in model.images(h, w, layout)[:2]:
                p = model.pixel_codes(img, layout)
                got = model.convert_codes(p, layout, siting, matrix, rng)
                exp, raw = model.convert_float(p, layout, siting, matrix, rng)
                for g, e, r in zip(got, exp, raw):
                    d = g - e
                    assert np.abs(d).max() <= 1
                    dist = np.abs(r - np.floor(r) - 0.5)
                    assert (dist[d != 0] <= bound).all(), float(dist[d != 0].max())


# ---- accumulators ----------------------------------------------------------------------------------------------------------------------------

def _row_bounds(row, k, x):
    pos, neg = sum(c for c in row if c > 0), sum(c for c in row if c < 0)
    return k + neg * x, k + pos * x


def test_accumulator_bounds_of_all_eight_matrices():
    """The header's admission rule for every row of the eight shipped matrices, both chroma geometries of the 8-bit ones: K + N * X >= 0 and
    K + P * X < 2^31; the largest chroma accumulator is 0.0625 * 2^31 (8-bit) and 0.25 * 2^31 (10-bit)."""
    worst8 = worst10 = 0
    for key, m in model.MATRICES8.items():
        off = model.OFFSETS8[key[1]]
        lo, hi = _row_bounds(m[0], (off[0] << 16) + (1 << 15), 255)
        assert 0 <= lo and hi < 2 ** 31
        for csh, x in ((19, 8 * 255), (18, 4 * 255)):
            for r in (1, 2):
                lo, hi = _row_bounds(m[r], (off[r] << csh) + (1 << (csh - 1)), x)
                assert 0 <= lo and hi < 2 ** 31, (key, r, csh)
                worst8 = max(worst8, hi)
    for key, m in model.MATRICES10.items():
        off = model.OFFSETS10[key[1]]
        lo, hi = _row_bounds(m[0], (off[0] << 16) + (1 << 15), 1020)
        assert 0 <= lo and hi < 2 ** 31
        for r in (1, 2):
            lo, hi = _row_bounds(m[r], (off[r] << 19) + (1 << 18), 8 * 1020)
            assert 0 <= lo and hi < 2 ** 31, (key, r)
            worst10 = max(worst10, hi)
    assert 0.0624 * 2 ** 31 < worst8 <= 0.0625 * 2 ** 31 + 2 ** 18 and 0.249 * 2 ** 31 < worst10 <= 0.25 * 2 ** 31, (worst8 / 2 ** 31, worst10 / 2 ** 31)
    # ... and the model's accumulators stay there on the corner frames (it asserts so itself)
    for layout in ("nv12", "uyvy422", "p010le"):
        for matrix, rng in model.CASES:
            for img in model.images(6, 8, layout)[1:]:
                model.pack(img, layout, "left", matrix, rng)


# ---- round trip through the sited source model ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ("nv12", "uyvy422", "p010le"))
def test_round_trip_through_the_sited_source_at_left(layout):
    """A frame whose channels are linear in x and constant in y — chroma-smooth — through the "left" egress model and back through
    tests/sited_model.py at "left".  In exact arithmetic the trip is the identity in the interior: [1 2 1] / 4 gives the chroma of column
    2 cx, the source hands it back at even columns and the mean of two neighbours — the linear function again — at odd ones, the rows are
    equal, and the float matrices are inverses.  The two stated roundings: the egress rounds each of Y, U, V to a sample (at most 0.5) and
    its integer matrix moves them by at most d_e = 3 * max * 2^-16 (the restatement test); the source's interpolation of samples carrying
    at most that error carries no more (its weights are positive and sum to one); its float matrix row k amplifies the three errors by
    |f[k][0]| + |f[k][1]| + |f[k][2]|; and the source rounds once more (0.5) and its integer matrix moves the result by at most d_s =
    3 * max * 2^-16.  So |out - in|[k] <= sum_j |f[k][j]| * (0.5 + d_e) + 0.5 + d_s, plus what the float matrices lack of being inverses
    (measured from the float matrices alone, times the largest code).  The errors are integers, so the floor of that.  The same trip with
    centre egress puts chroma half a pixel off and breaks the bound."""
    h, w = 6, 48
    deep = layout in model.DEEP
    x = np.arange(w, dtype=np.int64)
    codes = np.broadcast_to(np.stack([10 + 5 * x, 245 - 5 * x, 8 + 5 * x], axis=-1) * (4 if deep else 1), (h, w, 3)).copy()
    assert codes.min() >= 0 and codes.max() <= (1020 if deep else 255)
    img = deep_model.to_half(codes) if deep else codes.astype(np.uint8)
    fwd = model.float_matrix(layout, "bt601", "tv")
    inv = deep_model.rgb_float_matrix("bt601", "tv") if deep else unpack_model.float_matrix("bt601", "tv")
    d_e, d_s = 3 * (1020 if deep else 255) * 2.0 ** -16, 3 * (1023 if deep else 255) * 2.0 ** -16
    lack = np.abs(inv @ fwd - np.eye(3)).sum(axis=1) * (1020 if deep else 255)
    bound = np.floor(np.abs(inv).sum(axis=1) * (0.5 + d_e) + 0.5 + d_s + lack)
    assert lack.max() < 1e-9 and (bound >= 1).all() and (bound <= 3).all(), (bound, lack)
    inner = slice(2, w - 2)

    def trip(siting):
        packed = model.pack(img, layout, siting)
        back = sited_model.codes(packed, h, w, layout, "left")
        return np.abs(back - codes)[:, inner].reshape(-1, 3).max(axis=0)
    left, center = trip("left"), trip("center")
    assert (left <= bound).all(), (left, bound)
    assert (center > bound).any(), (center, bound)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------

def test_header_prototypes_are_the_bound_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_egress_sited_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(_lib.EGRESS_SITED_SYMBOLS) and len(protos) == 7, set(protos) ^ set(_lib.EGRESS_SITED_SYMBOLS)
    others = (set(_lib.SYMBOLS) | set(_lib.INGEST_SYMBOLS) | set(_lib.EGRESS_SYMBOLS) | set(_lib.UNPACK_SYMBOLS) | set(_lib.DEEP_SYMBOLS) | set(_lib.YUV422_SYMBOLS)
              | set(_lib.DEEP444_SYMBOLS) | set(_lib.SITED_SYMBOLS))
    assert not set(_lib.EGRESS_SITED_SYMBOLS) & others and _lib.EGRESS_SITED_SYMBOLS == _lib.stage_symbols("egress_sited")
    for name, args in protos.items():
        assert len(args.split(",")) == len(_lib.EGRESS_SITED_SYMBOLS[name][1]), name
        assert _lib.EGRESS_SITED_SYMBOLS[name] == _lib.EGRESS_SYMBOLS[name.replace("crtfx_egress_sited_", "crtfx_egress_")], name
        assert _lib.EGRESS_SITED_SYMBOLS[name] == _lib.SITED_SYMBOLS[name.replace("crtfx_egress_sited_", "crtfx_sited_")], name
    assert re.search(r'#include "crtfx_sited.h"', hdr) and "enum crtfx_sited_layout" not in hdr and "enum crtfx_sited_siting" not in hdr
    assert re.search(r"CRTFX_EGRESS_SITED_OPT_FORCE_GENERAL\s*=\s*1\s*,\s*CRTFX_EGRESS_SITED_OPT_SITING\s*=\s*2", hdr)
    assert (_lib.EGRESS_SITED_OPT_FORCE_GENERAL, _lib.EGRESS_SITED_OPT_SITING) == (1, 2)
    assert all(os.path.basename(f) in {os.path.basename(s) for s in _lib.SOURCES} for f in ("crtfx_egress_sited.hip", "crtfx_egress_sited.h"))
    assert all(os.path.exists(s) for s in _lib.SOURCES)
    assert "crtfx_egress_sited" in _lib.STAGE_UNITS
    lib = _lib.load()
    for name in _lib.EGRESS_SITED_SYMBOLS:
        assert getattr(lib, name).argtypes == _lib.EGRESS_SITED_SYMBOLS[name][1]
    import pythoncrt_amd as pc
    from pythoncrt_amd import _stage
    assert pc.EgressSited.__name__ in pc.__all__ and issubclass(pc.EgressSited, _stage.EgressPlan)
    assert pc.EgressSited._family == "egress_sited" and pc.EgressSited._layouts is pc.UnpackSited._layouts


def _create(lib, layout=_lib.SITED_NV12, h=12, w=20, pix_fmt=None, device=0, m=None, off=None, null=False, null_off=False):
    deep = layout in (_lib.SITED_YUV420P10LE, _lib.SITED_P010LE)
    tm, toff = (tables.yuv_matrix10 if deep else tables.yuv_matrix)("bt601", "tv")
    m = tm if m is None else np.ascontiguousarray(m, dtype=np.int32)
    off = toff if off is None else np.ascontiguousarray(off, dtype=np.int32)
    pix_fmt = (_lib.PIX_F16 if deep else _lib.PIX_U8) if pix_fmt is None else pix_fmt
    plan = ctypes.c_void_p(1)
    rc = lib.crtfx_egress_sited_create(device, h, w, pix_fmt, layout, None if null else tables.ptr(m), None if null_off else tables.ptr(off), ctypes.byref(plan))
    return rc, plan, (lib.crtfx_egress_sited_last_error(None) or b"").decode()


def test_create_refuses_bad_arguments_before_it_touches_a_device():
    """The argument checks come first, so they hold on any machine.  The pixel format follows from the layout: the other one is
    UNSUPPORTED, anything else INVALID; sizes, layouts, null tables, offsets and a matrix one step past the header's admission rule are
    INVALID; each leaves *out_plan NULL and a message.  A matrix on the rule's boundary is admitted."""
    lib = _lib.load()
    good8, good10 = tables.yuv_matrix("bt601", "tv")[0], tables.yuv_matrix10("bt601", "tv")[0]

    def edge(off, csh, x):
        """(the largest sum of positive entries, the largest magnitude of the sum of negative ones) a chroma row may have"""
        k = (off << csh) + (1 << (csh - 1))
        p, n = (2 ** 31 - 1 - k) // x, k // x
        assert k + p * x < 2 ** 31 <= k + (p + 1) * x and k - n * x >= 0 > k - (n + 1) * x
        return p, n
    p420, n420 = edge(128, 19, 8 * 255)
    p422, n422 = edge(128, 18, 4 * 255)
    p10, n10 = edge(512, 19, 8 * 1020)
    ky = (16 << 16) + (1 << 15)
    py, ny = (2 ** 31 - 1 - ky) // 255, ky // 255

    def with_row(good, r, row):
        m = good.copy()
        m[3 * r:3 * r + 3] = row
        return m
    inside = [dict(m=with_row(good8, 1, (p420 - 5, -n420, 5))), dict(m=with_row(good8, 2, (-(n420 - 1), p420, -1))), dict(m=with_row(good8, 0, (py, -ny, 0))),
              dict(layout=_lib.SITED_UYVY422, m=with_row(good8, 1, (p422, -n422, 0))), dict(layout=_lib.SITED_YUV422P, m=with_row(good8, 2, (0, -n422, p422))), dict(layout=_lib.SITED_YUV422P, m=with_row(good8, 1, (p420, 0, 0))),
              dict(layout=_lib.SITED_P010LE, m=with_row(good10, 1, (p10, 0, -n10))), dict(layout=_lib.SITED_YUV420P10LE, m=with_row(good10, 2, (-n10, p10 - 1, 1)))]
    outside = [dict(m=with_row(good8, 1, (p420 - 4, 0, 5))), dict(m=with_row(good8, 2, (0, -(n420 + 1), 0))), dict(m=with_row(good8, 0, (py + 1, 0, 0))),
               dict(m=with_row(good8, 0, (0, -ny, -1))), dict(layout=_lib.SITED_UYVY422, m=with_row(good8, 1, (p422 + 1, 0, 0))),
               dict(layout=_lib.SITED_YUYV422, m=with_row(good8, 2, (-n422, 0, -1))), dict(m=with_row(good8, 1, (p422, 0, 0))),
               dict(layout=_lib.SITED_P010LE, m=with_row(good10, 1, (p10 + 1, 0, 0))), dict(layout=_lib.SITED_YUV420P10LE, m=with_row(good10, 2, (-n10, 0, -1)))]
    assert p420 < p422                                                               # the 4:2:2 rule is its own: what it admits, 4:2:0 may refuse (above)
    cases = [(dict(pix_fmt=_lib.PIX_F16), _lib.E_UNSUPPORTED, "uint8"), (dict(layout=_lib.SITED_UYVY422, pix_fmt=_lib.PIX_F16), _lib.E_UNSUPPORTED, "uint8"),
             (dict(layout=_lib.SITED_P010LE, pix_fmt=_lib.PIX_U8), _lib.E_UNSUPPORTED, "half"),
             (dict(layout=_lib.SITED_YUV420P10LE, pix_fmt=_lib.PIX_U8), _lib.E_UNSUPPORTED, "half"),
             (dict(pix_fmt=7), _lib.E_INVALID, "pixel format"), (dict(layout=_lib.SITED_P010LE, pix_fmt=-1), _lib.E_INVALID, "pixel format"),
             (dict(h=0), _lib.E_INVALID, "size"), (dict(w=0), _lib.E_INVALID, "size"), (dict(w=32768), _lib.E_INVALID, "size"), (dict(h=32768), _lib.E_INVALID, "size"),
             (dict(layout=7), _lib.E_INVALID, "layout"), (dict(layout=-1), _lib.E_INVALID, "layout"), (dict(layout=7, pix_fmt=_lib.PIX_F16), _lib.E_INVALID, "layout"),
             (dict(null=True), _lib.E_INVALID, "null"), (dict(null_off=True), _lib.E_INVALID, "null"),
             (dict(off=(16, 256, 128)), _lib.E_INVALID, "offset"), (dict(off=(-1, 128, 128)), _lib.E_INVALID, "offset"),
             (dict(layout=_lib.SITED_P010LE, off=(64, 512, 1024)), _lib.E_INVALID, "offset")]
    cases += [(kw, _lib.E_INVALID, "accumulator") for kw in outside]
    for kw, code, word in cases:
        rc, plan, msg = _create(lib, **kw)
        assert rc == code and not plan.value and word in msg, (kw, rc, plan.value, msg)
    ok = inside + [dict(h=32767, w=32767)] + [dict(layout=i) for i in range(7)]
    for kw in ok:
        rc, plan, msg = _create(lib, **kw)
        assert rc in (_lib.OK, _lib.E_HIP), (kw, rc, msg)             # no device here: E_HIP; with one: a plan
        if rc == _lib.OK:
            assert lib.crtfx_egress_sited_destroy(plan) == _lib.OK
    assert lib.crtfx_egress_sited_create(0, 12, 20, _lib.PIX_U8, _lib.SITED_NV12, tables.ptr(good8), tables.ptr(tables.yuv_matrix("bt601", "tv")[1]), None) == _lib.E_INVALID
    assert b"out_plan" in lib.crtfx_egress_sited_last_error(None)
    assert lib.crtfx_egress_sited_destroy(None) == _lib.OK and lib.crtfx_egress_sited_set_option(None, 1, 1) == _lib.E_INVALID
    assert lib.crtfx_egress_sited_set_option(None, 2, 1) == _lib.E_INVALID
    assert lib.crtfx_egress_sited_run(None, None, 0, None, 0, 1, None) == _lib.E_INVALID and lib.crtfx_egress_sited_frame_bytes(None) == 0
    assert lib.crtfx_egress_sited_last_plan(None, ctypes.create_string_buffer(8), 8) == _lib.E_INVALID


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
    from pythoncrt_amd import EgressSited
    with pytest.raises(ValueError) as e:
        EgressSited("cuda", (8, 8), "nv12", siting="top-left")
    assert "siting" in str(e.value)
    with pytest.raises(ValueError):
        EgressSited("cpu", (8, 8), "nv12")


# ---- refusals of process_frames and the CLI -----------------------------------------------------------------------------------------------------

def test_process_frames_refuses_out_chroma_before_it_touches_a_device():
    import pythoncrt_amd as pc

    def never():
        raise AssertionError("a frame was read")
        yield

    def call(**kw):
        return pc.process_frames(never(), lambda a: (_ for _ in ()).throw(AssertionError("written")), 64, 36, 30.0, 1, **kw)
    cases = [dict(out_chroma="top-left"), dict(out_chroma="replicate", out_pix_fmt="nv12"), dict(out_chroma=None), dict(out_chroma="left"),
             dict(out_chroma="left", out_pix_fmt="rgb24", in_pix_fmt="nv12"), dict(out_chroma="left", in_pix_fmt="yuv444p10le", out_pix_fmt="yuv444p10le"),
             dict(out_chroma="left", in_pix_fmt="p010le", out_pix_fmt="gbrp10le"), dict(out_chroma="left", in_pix_fmt="x2rgb10le", out_pix_fmt="x2rgb10le")]
    for kw in cases:
        with pytest.raises(ValueError) as e:
            call(**kw)
        assert "out_chroma" in str(e.value), (kw, str(e.value))
    for kw, word in ((dict(out_chroma="left", out_pix_fmt="p010le"), "one end"), (dict(out_chroma="left", out_pix_fmt="nv12", in_pix_fmt="nv12", resize_on="host"), "host"),
                     (dict(out_chroma="left", in_pix_fmt="p010le", out_pix_fmt="p010le", in_size=(18, 32)), "in_size"),
                     (dict(out_chroma="left", out_pix_fmt="nv12", in_chroma="left"), "in_chroma")):
        with pytest.raises(ValueError) as e:                        # the refusals the other tests pin stay in front of a sited egress too
            call(**kw)
        assert word in str(e.value), (kw, str(e.value))


def test_cli_out_chroma_flag_and_refusals(monkeypatch, tmp_path, capsys):
    from pythoncrt_amd import cli
    parser = cli.add_input_flags(cli.add_output_flags(cli.build_parser()))
    assert parser.parse_args(["--input", "x"]).out_chroma == "center"
    for v in ("center", "left"):
        assert parser.parse_args(["--input", "x", "--out-chroma", v]).out_chroma == v
    with pytest.raises(SystemExit) as e:
        parser.parse_args(["--input", "x", "--out-chroma", "top-left"])
    assert e.value.code == 2
    assert "--out-chroma" in cli.__doc__ and "chroma_location=left" in cli.__doc__
    src = tmp_path / "in.raw"
    src.write_bytes(bytes(8 * 8 * 6))
    base = ["--input", str(src), "--output", str(tmp_path / "out.raw"), "--width", "8", "--height", "8"]
    for extra in (["--out-chroma", "left"], ["--out-chroma", "left", "--in-pix-fmt", "yuv444p10le", "--out-pix-fmt", "yuv444p10le"]):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code not in (0, None) and "--out-chroma" in str(e.value) and not (tmp_path / "out.raw").exists()
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:                            # the sharded CLI refuses the format as it does today
        cli.main(base + ["--out-pix-fmt", "nv12", "--out-chroma", "left"])
    assert "--out-pix-fmt nv12" in str(e.value) and "sharded" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(base + ["--out-chroma", "left"])
    assert "--out-chroma" in str(e.value) and not (tmp_path / "out.raw").exists()
    capsys.readouterr()


# ---- the kernel builds ----------------------------------------------------------------------------------------------------------------------------

def test_the_fourteen_kernel_builds_and_their_registers():
    """Exactly fourteen builds (seven layouts x two paths) in crtfx_egress_sited_impl, read from the library's code objects
    (tools/kernel_resources.py): no spills, no scratch, no LDS, no AGPRs, at most 128 registers — and the VGPR counts the header states."""
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n: v for n, v in res.items() if n.startswith("crtfx_egress_sited_impl::")}
    assert set(found) == {f"crtfx_egress_sited_impl::k_egress_sited<{l}, {p}>" for l in range(7) for p in (0, 1)}, sorted(found)
    text = open(HEADER).read()
    stated = {name: (int(v), int(g)) for name, v, g in re.findall(r"(\w+) (\d+) / (\d+)", text[text.index("Registers (gfx950"):text.index("no AGPRs")])}
    assert list(stated) == list(model.LAYOUTS), stated
    for name, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == 0 and v["agpr_count"] == 0 and v["vgpr_count"] + v["agpr_count"] <= 128, (name, v)
        layout, path = map(int, re.search(r"<(\d), (\d)>", name).groups())
        assert v["vgpr_count"] == stated[model.LAYOUTS[layout]][1 - path], (name, v["vgpr_count"], stated)
