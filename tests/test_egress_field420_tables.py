"""The field-paired 4:2:0 egress stage without a GPU: the tap tables and weights of tests/egress_field420_model.py written out, the four
consequences include/crtfx_egress_field420.h states (centre = the weave of the box models on the two fields, flat fields, a vertical ramp
at its siting, field independence), the integer model against its float64 restatement, the accumulator bounds and the admission boundary,
the C-ABI bound symbol for symbol and failing cleanly without a device, the refusals of the class, process_frames and the CLI with their
texts, the plans the ends build, and the eight kernel builds' registers."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pythoncrt_amd import _lib, _stage, tables  # noqa: E402
from tests import deep_model, yuv_model  # noqa: E402
from tests import egress_field420_model as model  # noqa: E402
from tests import egress_sited_model  # noqa: E402

HEADER = os.path.join(ROOT, "include", "crtfx_egress_field420.h")
SIZES = [(4, 1), (8, 7), (12, 16), (16, 24)]


# ---- tap tables and weights, written out ----------------------------------------------------------------------------------------------------

V_TAPS = {   # h: per chroma row (field, the frame rows of its four taps)
    4: [(0, (0, 0, 2, 2)), (1, (1, 1, 3, 3))],
    8: [(0, (0, 0, 2, 4)), (1, (1, 1, 3, 5)), (0, (2, 4, 6, 6)), (1, (3, 5, 7, 7))],
    12: [(0, (0, 0, 2, 4)), (1, (1, 1, 3, 5)), (0, (2, 4, 6, 8)), (1, (3, 5, 7, 9)), (0, (6, 8, 10, 10)), (1, (7, 9, 11, 11))],
}


def test_tap_tables_and_weights():
    for h, want in V_TAPS.items():
        assert model.v_taps(h) == want, h
    for h in (2, 5, 6, 10):
        with pytest.raises(AssertionError):
            model.v_taps(h)
    assert model.V_WEIGHTS == {"center": ((0, 8, 8, 0), (0, 8, 8, 0)), "left": ((3, 7, 5, 1), (1, 5, 7, 3))}
    assert model.H_WEIGHTS == {"left": (1, 2, 1), "center": (0, 2, 2)} and model.H_WEIGHTS is egress_sited_model.WEIGHTS
    assert all(sum(v) == 16 for pair in model.V_WEIGHTS.values() for v in pair) and all(sum(v) == 4 for v in model.H_WEIGHTS.values())
    # "left": the triangle of half-width two field rows around the siting, a quarter / three quarters of a field row below field row 2i
    for f, below in enumerate(model.SITING["left"]):
        assert [int(round(4 * (2 - abs(t - 1 - below)))) for t in range(4)] == list(model.V_WEIGHTS["left"][f]) and below == (0.25, 0.75)[f]
    # ... and the transpose of the (near, far) eighths by which the source stage (tests/field420_model.py) interpolates: field luma rows
    # 2i - 1 .. 2i + 2 take 3, 7, 5, 1 (top) and 1, 5, 7, 3 (bottom) eighths of their field's chroma row i
    from tests import field420_model
    cy, cyf, vn, vf = field420_model.v_taps(16, "left")
    for f in (0, 1):
        i = 1
        c = 2 * i + f
        eighths = [int(vn[y]) if cy[y] == c else int(vf[y]) if cyf[y] == c else 0 for y in range(2 * (2 * i - 1) + f, 2 * (2 * i + 2) + f + 1, 2)]
        assert tuple(eighths) == model.V_WEIGHTS["left"][f], (f, eighths)
    # S of single impulses: every sample's weights sum to 64 and every luma row feeds its own field only
    for chroma in model.CHROMAS:
        h, w = 8, 7
        acc = np.zeros((h // 2, (w + 1) // 2, 3), dtype=np.int64)
        for y in range(h):
            rows = np.zeros((h, w, 3), dtype=np.int64)
            rows[y] = 1
            s = model.filter_sum(rows, chroma)
            assert not s[(1 - (y & 1))::2].any(), (chroma, y)
            acc += s
        assert (acc == 64).all(), chroma
    assert model.LAYOUTS == ("yuv420p", "nv12", "yuv420p10le", "p010le") and model.CHROMAS == ("center", "left")
    from pythoncrt_amd import field420
    assert list(field420.LAYOUTS) == list(model.LAYOUTS) and list(field420.EGRESS_CHROMAS) == list(model.CHROMAS)
    assert [field420.EGRESS_CHROMAS[c] for c in model.CHROMAS] == [_lib.EGRESS_FIELD420_CENTER, _lib.EGRESS_FIELD420_LEFT] == [0, 1]
    for layout in model.LAYOUTS:
        for h, w in SIZES + [(1080, 1920)]:
            assert field420.frame_bytes(h, w, layout) == model.frame_bytes(h, w, layout)
        for matrix, rng in model.CASES:
            m, off, top = model.tables(layout, matrix, rng)
            tm, toff = (tables.yuv_matrix10 if layout in model.DEEP else tables.yuv_matrix)(matrix, rng)
            assert np.array_equal(m.reshape(-1), tm) and tuple(toff) == tuple(off)


# ---- the consequences the header states -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", model.LAYOUTS)
def test_center_is_the_weave_of_the_box_stages_on_the_two_fields(layout):
    """(v_t) = (0, 8, 8, 0), (wl, w0, wr) = (0, 2, 2): S is 16 times the box sum of the field and the shift has four more bits, so every
    byte is that of yuv_model.pack / deep_model.pack run on each field as an h/2 x w frame — all four matrices of the layout (eight over
    the two sample depths), four sizes, the three test images of the layout's family."""
    assert model.box.__module__ == model.__name__ and (deep_model.pack if layout in model.DEEP else yuv_model.pack)
    for h, w in SIZES:
        for i, img in enumerate(model.images(h, w, layout)):
            for matrix, rng in model.CASES:
                got, exp = model.pack(img, layout, "center", matrix, rng), model.weave_of_fields(img, layout, matrix, rng)
                assert got.dtype == exp.dtype == np.uint8 and got.shape == (model.frame_bytes(h, w, layout),) and np.array_equal(got, exp), (h, w, i, matrix, rng)
    p = np.random.default_rng(3).integers(0, 256, (8, 7, 3))
    box_sum = deep_model.box_sum if layout in model.DEEP else yuv_model.box_sum
    s = model.filter_sum(p, "center")
    for f in (0, 1):
        assert np.array_equal(s[f::2], 16 * box_sum(p[f::2]))


@pytest.mark.parametrize("chroma", model.CHROMAS)
@pytest.mark.parametrize("layout", model.LAYOUTS)
def test_two_flat_fields_give_the_box_bytes_of_each_field(layout, chroma):
    scale = 4 if layout in model.DEEP else 1
    colours = [(np.array(a) * scale, np.array(b) * scale) for a, b in (((200, 30, 90), (10, 250, 60)), ((255, 255, 255), (0, 0, 0)), ((0, 0, 255), (255, 0, 0)))]
    for h, w in SIZES:
        for matrix, rng in model.CASES:
            for top, bottom in colours:
                y, u, v = model.samples(model.pack(model.two_colour_frame(h, w, layout, top, bottom), layout, chroma, matrix, rng), h, w, layout)
                for f, colour in enumerate((top, bottom)):
                    flat = model.to_frame(np.broadcast_to(colour, (h, w, 3)), layout)
                    fy, fu, fv = model.samples(model.box(flat, layout, matrix, rng), h, w, layout)
                    assert np.array_equal(y[f::2], fy[f::2]) and np.array_equal(u[f::2], fu[f::2]) and np.array_equal(v[f::2], fv[f::2]), (h, w, f, matrix, rng)


def test_a_vertical_ramp_is_reproduced_at_the_sample_s_siting():
    """Field f holds p = a + b k on its row k (constant in x, so H = 4 p): S = 4 * sum v_t p(k_t) = 64 a + 4 b * sum v_t k_t.  Unclamped,
    sum v_t k_t = 16 (2 i) + 16 * siting, so S / 64 is the ramp at field row 2 i + siting: exactly.  The clamped first and last rows of a
    field, written out: the outer tap repeats its neighbour."""
    h, w = 24, 6
    n = h // 4                                                                       # chroma rows of a field
    a = (40, 200, 17)
    b = (8, -4, 12)
    k = np.arange(h // 2, dtype=np.int64)
    field = np.stack([a[c] + b[c] * k for c in range(3)], axis=-1)                   # [h / 2, 3]
    assert field.min() >= 0 and field.max() <= 255
    for f in (0, 1):
        other = np.random.default_rng(f).integers(0, 256, (h // 2, w, 3))
        p = np.empty((h, w, 3), dtype=np.int64)
        p[f::2] = field[:, None, :]
        p[1 - f::2] = other
        for chroma in model.CHROMAS:
            s = model.filter_sum(p, chroma)[f::2]                                   # the field's chroma rows, [n, cw, 3]
            sixteenths = int(16 * model.SITING[chroma][f])
            assert sixteenths == {("center", 0): 8, ("center", 1): 8, ("left", 0): 4, ("left", 1): 12}[(chroma, f)]
            for i in range(1, n - 1):
                for c in range(3):
                    assert (s[i, :, c] == 64 * a[c] + b[c] * (128 * i + 4 * sixteenths)).all(), (f, chroma, i, c)
                    assert (s[i, :, c] / 64.0 == a[c] + b[c] * (2 * i + model.SITING[chroma][f])).all()
            # clamped: first row taps (0, 0, 1, 2), last row taps (2i - 1, 2i, 2i + 1, 2i + 1)
            first = {("center", 0): 8, ("center", 1): 8, ("left", 0): 7, ("left", 1): 13}[(chroma, f)]              # sum v_t k_t
            last = {("center", 0): 8, ("center", 1): 8, ("left", 0): 3, ("left", 1): 9}[(chroma, f)]                # ... - 32 i
            for c in range(3):
                assert (s[0, :, c] == 64 * a[c] + 4 * b[c] * first).all(), (f, chroma, c)
                assert (s[n - 1, :, c] == 64 * a[c] + 4 * b[c] * (32 * (n - 1) + last)).all(), (f, chroma, c)


@pytest.mark.parametrize("layout", model.LAYOUTS)
def test_the_two_fields_are_independent(layout):
    """Complement only the bottom-field rows of a 16 x 24 random frame: no Y and no chroma sample of the top field changes, under both
    chroma values — while the progressive stage (tests/egress_sited_model.py) on the same pair of frames changes more than half of the
    chroma rows an interlaced decoder reads as the top field's (measured: 0.98)."""
    h, w = 16, 24
    top_code = 1020 if layout in model.DEEP else 255
    p = np.random.default_rng(5).integers(0, top_code + 1, (h, w, 3))
    q = p.copy()
    q[1::2] = top_code - q[1::2]
    a, b = model.to_frame(p, layout), model.to_frame(q, layout)
    for chroma in model.CHROMAS:
        ya, ua, va = model.samples(model.pack(a, layout, chroma), h, w, layout)
        yb, ub, vb = model.samples(model.pack(b, layout, chroma), h, w, layout)
        assert np.array_equal(ya[0::2], yb[0::2]) and np.array_equal(ua[0::2], ub[0::2]) and np.array_equal(va[0::2], vb[0::2])
        assert (ua[1::2] != ub[1::2]).mean() > 0.5 and (va[1::2] != vb[1::2]).mean() > 0.5 and (ya[1::2] != yb[1::2]).mean() > 0.5
        _, pa, qa = egress_sited_model.samples(egress_sited_model.pack(a, layout, chroma), h, w, layout)
        _, pb, qb = egress_sited_model.samples(egress_sited_model.pack(b, layout, chroma), h, w, layout)
        share = np.concatenate([(pa[0::2] != pb[0::2]).reshape(-1), (qa[0::2] != qb[0::2]).reshape(-1)]).mean()
        print(f"{layout} {chroma}: the progressive stage changes {share:.3f} of the top field's chroma samples")
        assert share > 0.5, (layout, chroma, float(share))


# ---- the integer model against the float restatement -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("matrix,rng", model.CASES)
@pytest.mark.parametrize("layout", ("nv12", "yuv420p10le"))
def test_model_against_the_float_restatement(layout, matrix, rng):
    """Random frames: the samples are the float64 ones except where the float value lies within 3 * max_sample * 2^-16 of a half-integer
    (tests/test_egress_sited_tables.py's bound), and there they differ by one.  Derived here as there, from the rounding of the integer
    matrix: the entries of a row differ from 65536 x the float ones by e0, e1, e2, the filtered value S / 64 of a channel is at most the
    largest per-pixel code (its weights are positive and sum to one), so the sums differ by at most (|e0| + |e1| + |e2|) * 2^-16 * max
    code — and |e0| + |e1| + |e2| <= 3 for every row of all eight matrices, asserted below.  The filter itself is exact in both: S is an
    integer below 2^17 and S / 64 is a float64 without rounding."""
    top_code = 1020 if layout in model.DEEP else 255
    bound = 3 * (1023 if layout in model.DEEP else 255) * 2.0 ** -16
    m, _, _ = model.tables(layout, matrix, rng)
    err = np.abs(m - 65536.0 * model.float_matrix(layout, matrix, rng)).sum(axis=1)
    assert (err <= 3.0).all() and err.max() * top_code * 2.0 ** -16 <= bound, err
    for chroma in model.CHROMAS:
        for h, w in ((16, 33), (32, 64)):
            for img in model.images(h, w, layout)[:2]:
                p = model.pixel_codes(img, layout)
                got = model.convert_codes(p, layout, chroma, matrix, rng)
                exp, raw = model.convert_float(p, layout, chroma, matrix, rng)
                for g, e, r in zip(got, exp, raw):
                    d = g - e
                    assert np.abs(d).max() <= 1
                    dist = np.abs(r - np.floor(r) - 0.5)
                    assert (dist[d != 0] <= bound).all(), float(dist[d != 0].max())


# ---- accumulators ----------------------------------------------------------------------------------------------------------------------------

def _row_bounds(row, k, x):
    pos, neg = sum(int(c) for c in row if c > 0), sum(int(c) for c in row if c < 0)
    return k + neg * x, k + pos * x


def test_accumulator_bounds_of_all_eight_matrices():
    """The header's admission rules for every row of the eight shipped matrices.  8-bit chroma: [0, 2^31), at most 0.5 * 2^31.  10-bit
    chroma: past int32 — 1.876 * 2^31 (limited range), 1.99999 * 2^31 (full range) — but inside [0, 2^32), and at least 0.002 * 2^31."""
    for key, m in model.MATRICES8.items():
        off = model.OFFSETS8[key[1]]
        lo, hi = _row_bounds(m[0], (off[0] << 16) + (1 << 15), 255)
        assert 0 <= lo and hi < 2 ** 31
        for r in (1, 2):
            lo, hi = _row_bounds(m[r], (off[r] << 22) + (1 << 21), 64 * 255)
            assert 0 <= lo and hi <= 0.5 * 2 ** 31 and model.limit("nv12") == 2 ** 31, (key, r, lo, hi)
    worst = {"tv": 0, "pc": 0}
    least = 2 ** 32
    for key, m in model.MATRICES10.items():
        off = model.OFFSETS10[key[1]]
        lo, hi = _row_bounds(m[0], (off[0] << 16) + (1 << 15), 1020)
        assert 0 <= lo and hi < 2 ** 31
        for r in (1, 2):
            lo, hi = _row_bounds(m[r], (off[r] << 22) + (1 << 21), 64 * 1020)
            assert 0 <= lo and 2 ** 31 < hi < 2 ** 32 == model.limit("p010le"), (key, r, lo, hi)
            worst[key[1]] = max(worst[key[1]], hi)
            least = min(least, lo)
    assert 1.8759 * 2 ** 31 < worst["tv"] < 1.8760 * 2 ** 31 and 1.99998 * 2 ** 31 < worst["pc"] < 2 ** 32, {k: v / 2 ** 31 for k, v in worst.items()}
    assert 0.0019 * 2 ** 31 < least < 0.002 * 2 ** 31 + 2 ** 16, least / 2 ** 31


@pytest.mark.parametrize("layout", ("yuv420p10le", "p010le"))
def test_the_frame_that_drives_a_10_bit_accumulator_to_its_maximum(layout):
    """1020 in the channels with positive entries and 0 in the others: every accumulator of the row is K + P * X, above 2^31, and the
    model (which asserts [0, 2^32) itself) gives the sample the float restatement gives."""
    for matrix, rng in model.CASES:
        m, off, top = model.tables(layout, matrix, rng)
        for row in (1, 2):
            k = (off[row] << 22) + (1 << 21)
            for low in (False, True):
                img = model.extreme_frame(8, 16, layout, row, matrix, rng, low)
                p = model.pixel_codes(img, layout)
                assert set(np.unique(p)) <= {0, 1020}
                for chroma in model.CHROMAS:
                    acc = model.accumulators(p, layout, chroma, matrix, rng)[row]
                    want = _row_bounds(m[row], k, 64 * 1020)[0 if low else 1]
                    assert (acc == want).all() and (low or want > 2 ** 31), (matrix, rng, row, low, chroma)
                    got = model.convert_codes(p, layout, chroma, matrix, rng)
                    exp, _ = model.convert_float(p, layout, chroma, matrix, rng)
                    assert all(np.abs(g - e).max() <= 1 for g, e in zip(got, exp))
                    assert (got[row] == min(want >> 22, top)).all()


@pytest.mark.parametrize("layout", model.LAYOUTS)
def test_a_matrix_on_each_side_of_the_admission_boundary(layout):
    """The U row with the largest sums the rule admits: the extreme frames reach K + P * X = limit - (less than X) and K + N * X < X and
    the model holds; one more unit in a positive entry and the model's own assertion fails on the same frame."""
    inside, outside = model.boundary_matrix(layout)
    lim = model.limit(layout)
    x = 64 * (1020 if layout in model.DEEP else 255)
    top_code = x // 64
    high = model.to_frame(np.broadcast_to(np.array([top_code, 0, top_code]), (4, 8, 3)), layout)
    lowf = model.to_frame(np.broadcast_to(np.array([0, top_code, 0]), (4, 8, 3)), layout)
    for chroma in model.CHROMAS:
        acc = model.accumulators(model.pixel_codes(high, layout), layout, chroma, m=inside)[1]
        assert (acc == acc.flat[0]).all() and lim - x <= acc.flat[0] < lim
        acc = model.accumulators(model.pixel_codes(lowf, layout), layout, chroma, m=inside)[1]
        assert (acc == acc.flat[0]).all() and 0 <= acc.flat[0] < x
        model.pack(high, layout, chroma, m=inside)
        model.pack(lowf, layout, chroma, m=inside)
        with pytest.raises(AssertionError):
            model.pack(high, layout, chroma, m=outside)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------

def test_header_prototypes_are_the_bound_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_egress_field420_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(_lib.EGRESS_FIELD420_SYMBOLS) and len(protos) == 7, set(protos) ^ set(_lib.EGRESS_FIELD420_SYMBOLS)
    others = (set(_lib.SYMBOLS) | set(_lib.INGEST_SYMBOLS) | set(_lib.EGRESS_SYMBOLS) | set(_lib.UNPACK_SYMBOLS) | set(_lib.DEEP_SYMBOLS) | set(_lib.YUV422_SYMBOLS)
              | set(_lib.DEEP444_SYMBOLS) | set(_lib.SITED_SYMBOLS) | set(_lib.EGRESS_SITED_SYMBOLS) | set(_lib.FIELD420_SYMBOLS))
    assert not set(_lib.EGRESS_FIELD420_SYMBOLS) & others and _lib.EGRESS_FIELD420_SYMBOLS == _lib.stage_symbols("egress_field420")
    for name, args in protos.items():
        assert len(args.split(",")) == len(_lib.EGRESS_FIELD420_SYMBOLS[name][1]), name
        assert _lib.EGRESS_FIELD420_SYMBOLS[name] == _lib.EGRESS_SITED_SYMBOLS[name.replace("crtfx_egress_field420_", "crtfx_egress_sited_")], name
    assert re.search(r'#include "crtfx_field420.h"', hdr) and "enum crtfx_field420_layout" not in hdr
    assert re.search(r"CRTFX_EGRESS_FIELD420_OPT_FORCE_GENERAL\s*=\s*1\s*,\s*CRTFX_EGRESS_FIELD420_OPT_CHROMA\s*=\s*2", hdr)
    assert re.search(r"CRTFX_EGRESS_FIELD420_CENTER\s*=\s*0\s*,\s*CRTFX_EGRESS_FIELD420_LEFT\s*=\s*1", hdr)
    assert (_lib.EGRESS_FIELD420_OPT_FORCE_GENERAL, _lib.EGRESS_FIELD420_OPT_CHROMA, _lib.EGRESS_FIELD420_CENTER, _lib.EGRESS_FIELD420_LEFT) == (1, 2, 0, 1)
    assert all(os.path.basename(f) in {os.path.basename(s) for s in _lib.SOURCES} for f in ("crtfx_egress_field420.hip", "crtfx_egress_field420.h"))
    assert all(os.path.exists(s) for s in _lib.SOURCES)
    assert "crtfx_egress_field420" in _lib.STAGE_UNITS
    lib = _lib.load()
    for name in _lib.EGRESS_FIELD420_SYMBOLS:
        assert getattr(lib, name).argtypes == _lib.EGRESS_FIELD420_SYMBOLS[name][1]
    import pythoncrt_amd as pc
    assert pc.EgressField420.__name__ in pc.__all__ and issubclass(pc.EgressField420, _stage.EgressPlan)
    assert pc.EgressField420._family == "egress_field420" and pc.EgressField420._layouts is pc.UnpackField420._layouts
    assert "h % 4 == 2 is deliberately NOT served" in open(HEADER).read()


def _create(lib, layout=_lib.FIELD420_NV12, h=12, w=20, pix_fmt=None, device=0, m=None, off=None, null=False, null_off=False):
    deep = layout in (_lib.FIELD420_YUV420P10LE, _lib.FIELD420_P010LE)
    tm, toff = (tables.yuv_matrix10 if deep else tables.yuv_matrix)("bt601", "tv")
    m = tm if m is None else np.ascontiguousarray(np.asarray(m).reshape(-1), dtype=np.int32)
    off = toff if off is None else np.ascontiguousarray(off, dtype=np.int32)
    pix_fmt = (_lib.PIX_F16 if deep else _lib.PIX_U8) if pix_fmt is None else pix_fmt
    plan = ctypes.c_void_p(1)
    rc = lib.crtfx_egress_field420_create(device, h, w, pix_fmt, layout, None if null else tables.ptr(m), None if null_off else tables.ptr(off), ctypes.byref(plan))
    return rc, plan, (lib.crtfx_egress_field420_last_error(None) or b"").decode()


def test_create_refuses_bad_arguments_before_it_touches_a_device():
    """The argument checks come first, so they hold on any machine.  A height that is no multiple of 4 (2, 6, 5), a width of 0, the other
    pixel format (UNSUPPORTED), an unknown one, null tables, offsets and a matrix one step past the header's admission rule: each leaves
    *out_plan NULL and a message.  A matrix on the rule's boundary is admitted."""
    lib = _lib.load()
    good8, good10 = tables.yuv_matrix("bt601", "tv")[0], tables.yuv_matrix10("bt601", "tv")[0]
    in8, out8 = model.boundary_matrix("nv12")
    in10, out10 = model.boundary_matrix("p010le")
    assert in10[1][0] > 2 ** 15 and in8[1][0] > in10[1][0] and in10[1][1] < 0
    ky = (16 << 16) + (1 << 15)
    py, ny = (2 ** 31 - 1 - ky) // 255, ky // 255

    def with_row(good, r, row):
        m = np.array(good).reshape(-1).copy()
        m[3 * r:3 * r + 3] = row
        return m
    cases = [(dict(h=2), _lib.E_INVALID, "below 4"), (dict(h=6), _lib.E_INVALID, "multiple of 4"), (dict(h=5), _lib.E_INVALID, "multiple of 4"),
             (dict(h=10, layout=_lib.FIELD420_P010LE), _lib.E_INVALID, "multiple of 4"), (dict(h=0), _lib.E_INVALID, "size"), (dict(h=-4), _lib.E_INVALID, "size"),
             (dict(w=0), _lib.E_INVALID, "size"), (dict(w=32768), _lib.E_INVALID, "size"), (dict(h=32768), _lib.E_INVALID, "size"),
             (dict(pix_fmt=_lib.PIX_F16), _lib.E_UNSUPPORTED, "uint8"), (dict(layout=_lib.FIELD420_YUV420P, pix_fmt=_lib.PIX_F16), _lib.E_UNSUPPORTED, "uint8"),
             (dict(layout=_lib.FIELD420_P010LE, pix_fmt=_lib.PIX_U8), _lib.E_UNSUPPORTED, "half"),
             (dict(layout=_lib.FIELD420_YUV420P10LE, pix_fmt=_lib.PIX_U8), _lib.E_UNSUPPORTED, "half"),
             (dict(pix_fmt=7), _lib.E_INVALID, "pixel format"), (dict(layout=_lib.FIELD420_P010LE, pix_fmt=-1), _lib.E_INVALID, "pixel format"),
             (dict(layout=4), _lib.E_INVALID, "layout"), (dict(layout=-1), _lib.E_INVALID, "layout"),
             (dict(null=True), _lib.E_INVALID, "null"), (dict(null_off=True), _lib.E_INVALID, "null"),
             (dict(off=(16, 256, 128)), _lib.E_INVALID, "offset"), (dict(off=(-1, 128, 128)), _lib.E_INVALID, "offset"),
             (dict(layout=_lib.FIELD420_P010LE, off=(64, 512, 1024)), _lib.E_INVALID, "offset"),
             (dict(m=out8), _lib.E_INVALID, "accumulator"), (dict(layout=_lib.FIELD420_YUV420P, m=out8), _lib.E_INVALID, "accumulator"),
             (dict(layout=_lib.FIELD420_P010LE, m=out10), _lib.E_INVALID, "accumulator"), (dict(layout=_lib.FIELD420_YUV420P10LE, m=out10), _lib.E_INVALID, "accumulator"),
             (dict(layout=_lib.FIELD420_P010LE, m=with_row(good10, 2, in8[1])), _lib.E_INVALID, "accumulator"),      # what 8 bits admit, 10 bits need not: X is four times theirs
             (dict(m=with_row(good8, 0, (py + 1, 0, 0))), _lib.E_INVALID, "accumulator"), (dict(m=with_row(good8, 0, (0, -ny, -1))), _lib.E_INVALID, "accumulator"),
             (dict(layout=_lib.FIELD420_P010LE, m=with_row(good10, 2, (0, int(in10[1][1]) - 1, 0))), _lib.E_INVALID, "accumulator")]
    for kw, code, word in cases:
        rc, plan, msg = _create(lib, **kw)
        assert rc == code and not plan.value and word in msg, (kw, rc, plan.value, msg)
    ok = [dict(m=in8), dict(layout=_lib.FIELD420_P010LE, m=in10), dict(layout=_lib.FIELD420_YUV420P10LE, m=with_row(good10, 2, in10[1])),
          dict(m=with_row(good8, 0, (py, -ny, 0))), dict(h=32764, w=32767), dict(h=4, w=1)] + [dict(layout=i) for i in range(4)]
    for kw in ok:
        rc, plan, msg = _create(lib, **kw)
        assert rc in (_lib.OK, _lib.E_HIP), (kw, rc, msg)             # no device here: E_HIP; with one: a plan
        if rc == _lib.OK:
            assert lib.crtfx_egress_field420_destroy(plan) == _lib.OK
    assert lib.crtfx_egress_field420_create(0, 12, 20, _lib.PIX_U8, _lib.FIELD420_NV12, tables.ptr(good8), tables.ptr(tables.yuv_matrix("bt601", "tv")[1]), None) == _lib.E_INVALID
    assert b"out_plan" in lib.crtfx_egress_field420_last_error(None)
    assert lib.crtfx_egress_field420_destroy(None) == _lib.OK and lib.crtfx_egress_field420_set_option(None, 1, 1) == _lib.E_INVALID
    assert lib.crtfx_egress_field420_set_option(None, 2, 1) == _lib.E_INVALID
    assert lib.crtfx_egress_field420_run(None, None, 0, None, 0, 1, None) == _lib.E_INVALID and lib.crtfx_egress_field420_frame_bytes(None) == 0
    assert lib.crtfx_egress_field420_last_plan(None, ctypes.create_string_buffer(8), 8) == _lib.E_INVALID


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
    from pythoncrt_amd import EgressField420
    with pytest.raises(ValueError) as e:
        EgressField420("cuda", (8, 8), "nv12", chroma="replicate")
    assert "chroma" in str(e.value)
    with pytest.raises(ValueError):
        EgressField420("cpu", (8, 8), "nv12")


# ---- refusals of process_frames and the CLI -----------------------------------------------------------------------------------------------------

FORMATS_420 = "(yuv420p, nv12, yuv420p10le, p010le)"
MEMBER_TEXT = "out_chroma_rows must be 'progressive' or 'interlaced', got {!r}"
FORMAT_TEXT = "out_chroma_rows='interlaced' with out_pix_fmt={!r}: only a 4:2:0 output has chroma rows that two fields share " + FORMATS_420
FORMAT_FLAGS = "--out-chroma-rows interlaced with --out-pix-fmt {}: only a 4:2:0 output has chroma rows that two fields share " + FORMATS_420
HEIGHT_TEXT = ("out_chroma_rows='interlaced': a delivered frame of {} row(s) has no two fields with whole pairs of luma rows under their chroma rows "
               "(a height that is a multiple of 4)")
HEIGHT_FLAGS = ("--out-chroma-rows interlaced with a delivery height of {0}: a frame of {0} row(s) has no two fields with whole pairs of luma rows "
                "under their chroma rows (a height that is a multiple of 4)")
# (keywords, (out_h, out_w), the text)
KEYWORD_CASES = [
    (dict(out_chroma_rows="field"), (36, 64), MEMBER_TEXT.format("field")),
    (dict(out_chroma_rows=None), (36, 64), MEMBER_TEXT.format(None)),
    (dict(out_chroma_rows=1, out_pix_fmt="nv12"), (36, 64), MEMBER_TEXT.format(1)),
    (dict(out_chroma_rows="interlaced"), (36, 64), FORMAT_TEXT.format("rgb24")),
    (dict(out_chroma_rows="interlaced", out_pix_fmt="yuv422p"), (36, 64), FORMAT_TEXT.format("yuv422p")),
    (dict(out_chroma_rows="interlaced", out_pix_fmt="uyvy422", deliver_interlace="tff"), (36, 64), FORMAT_TEXT.format("uyvy422")),
    (dict(out_chroma_rows="interlaced", out_pix_fmt="nv12"), (38, 64), HEIGHT_TEXT.format(38)),
    (dict(out_chroma_rows="interlaced", out_pix_fmt="yuv420p", out_chroma="left"), (7, 64), HEIGHT_TEXT.format(7)),
    (dict(out_chroma_rows="interlaced", out_pix_fmt="nv12", deliver_size=(18, 32)), (36, 64), HEIGHT_TEXT.format(18)),
    (dict(out_chroma_rows="interlaced", out_pix_fmt="p010le", in_pix_fmt="p010le"), (2, 64), HEIGHT_TEXT.format(2)),
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


def test_process_frames_refuses_before_it_touches_a_device(no_device):
    import pythoncrt_amd as pc
    for kw, (oh, ow), text in KEYWORD_CASES:
        with pytest.raises(ValueError) as e:
            pc.process_frames(_never(), lambda a: (_ for _ in ()).throw(AssertionError("written")), ow, oh, 30.0, 1, **kw)
        assert str(e.value) == text and e.value.rule.startswith("out_chroma_rows"), (kw, str(e.value))
    for fmt in ("yuv444p10le", "gbrp10le", "x2rgb10le"):
        with pytest.raises(ValueError) as e:
            pc.process_frames(_never(), lambda a: None, 64, 36, 30.0, 1, out_chroma_rows="interlaced", in_pix_fmt=fmt, out_pix_fmt=fmt)
        assert str(e.value) == FORMAT_TEXT.format(fmt)
    # the rules in front of it keep their place: RULES and FIELD_RULES are walked first
    for kw, word in ((dict(out_chroma_rows="interlaced", out_pix_fmt="p010le"), "one end"), (dict(out_chroma_rows="interlaced", out_chroma="left"), "out_chroma="),
                     (dict(out_chroma_rows="interlaced", in_chroma_rows="interlaced"), "in_chroma_rows="),
                     (dict(out_chroma_rows="interlaced", out_pix_fmt="nv12", deliver_lowpass="linear"), "deliver_lowpass")):
        with pytest.raises(ValueError) as e:
            pc.process_frames(_never(), lambda a: None, 64, 36, 30.0, 1, **kw)
        assert word in str(e.value), (kw, str(e.value))
    # what is no refusal reaches the device question: a multiple of 4, with and without a weave
    for kw in (dict(out_pix_fmt="nv12"), dict(out_pix_fmt="yuv420p", deliver_interlace="bff"), dict(out_pix_fmt="nv12", deliver_size=(20, 32))):
        with pytest.raises(AssertionError) as e:
            pc.process_frames(_never(), lambda a: None, 64, 36, 30.0, 1, out_chroma_rows="interlaced", **kw)
        assert "device was asked" in str(e.value)
    with pytest.raises(TypeError):
        pc.process_frames(_never(), lambda a: None, 64, 36, 30.0, 1, out_chroma_row="interlaced")


def test_the_cli_has_the_flag_and_its_refusals(no_device, monkeypatch, tmp_path, capsys):
    from pythoncrt_amd import cli
    parser = cli.add_input_flags(cli.add_output_flags(cli.build_parser()))
    assert parser.parse_args(["--input", "x"]).out_chroma_rows == "progressive"
    for v in ("progressive", "interlaced"):
        assert parser.parse_args(["--input", "x", "--out-chroma-rows", v]).out_chroma_rows == v
    with pytest.raises(SystemExit) as e:
        parser.parse_args(["--input", "x", "--out-chroma-rows", "field"])
    assert e.value.code == 2
    assert "--out-chroma-rows" in cli.__doc__ and "crtfx_egress_field420.h" in cli.__doc__
    src, out = tmp_path / "in.raw", tmp_path / "out.raw"
    src.write_bytes(bytes(8 * 8 * 6))

    def argv(h, *extra):
        return ["--input", str(src), "--width", "8", "--height", str(h), "--out-chroma-rows", "interlaced", *extra]
    cases = [(argv(8), FORMAT_FLAGS.format("rgb24")), (argv(8, "--out-pix-fmt", "yuyv422"), FORMAT_FLAGS.format("yuyv422")),
             (argv(8, "--out-pix-fmt", "gbrp10le", "--in-pix-fmt", "gbrp10le"), FORMAT_FLAGS.format("gbrp10le")),
             (argv(6, "--out-pix-fmt", "nv12"), HEIGHT_FLAGS.format(6)), (argv(7, "--out-pix-fmt", "yuv420p", "--out-chroma", "left"), HEIGHT_FLAGS.format(7)),
             (argv(8, "--out-pix-fmt", "nv12", "--deliver-width", "8", "--deliver-height", "10"), HEIGHT_FLAGS.format(10)),
             (argv(6, "--out-pix-fmt", "p010le", "--in-pix-fmt", "p010le"), HEIGHT_FLAGS.format(6))]
    for args, text in cases:
        with pytest.raises(SystemExit) as e:
            cli.main(args + ["--output", str(out)])
        assert e.value.code == text and getattr(e.value.__cause__, "rule", "").startswith("out_chroma_rows") and not out.exists(), (args, e.value.code)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:                            # early: in front of the sharded CLI's branch, which writes rgb24 only
        cli.main(argv(8) + ["--output", str(out)])
    assert e.value.code == FORMAT_FLAGS.format("rgb24") and not out.exists()
    with pytest.raises(SystemExit) as e:                            # ... and refuses the format itself, as it does today
        cli.main(argv(8, "--out-pix-fmt", "nv12") + ["--output", str(out)])
    assert "--out-pix-fmt nv12" in str(e.value.code) and "sharded" in str(e.value.code) and not out.exists()
    capsys.readouterr()


# the keywords of process_frames that a Raw holds
_RAW = ("resize_on", "out_pix_fmt", "out_matrix", "out_range", "in_pix_fmt", "in_matrix", "in_range", "in_size", "in_chroma", "out_chroma",
        "deliver_size", "in_filter", "deliver_filter", "in_crop", "deliver_fit", "deliver_pad_color", "chain_pix", "dither", "deinterlace",
        "field_order", "deinterlace_fields", "in_lut", "deliver_lut", "deliver_interlace", "deliver_lowpass", "in_signal", "signal_chroma",
        "signal_crawl", "in_chroma_rows", "out_chroma_rows")


def _defaults():
    """Each of them at the default of process_frames' signature."""
    import inspect
    import pythoncrt_amd as pc
    sig = inspect.signature(pc.process_frames).parameters
    return {n: sig[n].default for n in _RAW}


def test_out_field_rules_fire_on_the_surfaces_they_speak_on():
    """OUT_FIELD_RULES is a table of its own behind RULES and FIELD_RULES, which stay as they were: three entries, all in front of the
    sharded branch; the membership check speaks to the keywords only, the other two to both surfaces."""
    from pythoncrt_amd import options
    defaults = _defaults()
    assert defaults["out_chroma_rows"] == "progressive"
    assert [r.name for r in options.OUT_FIELD_RULES] == ["out_chroma_rows", "out_chroma_rows_format", "out_chroma_rows_height"]
    assert all(type(r) is options.Rule and r.early for r in options.OUT_FIELD_RULES)
    assert [(r.keywords is not None, r.flags is not None) for r in options.OUT_FIELD_RULES] == [(True, False), (True, True), (True, True)]
    assert [r.name for r in options.FIELD_RULES] == ["in_chroma_rows", "in_chroma_rows_format", "in_chroma_rows_height"]
    assert len(options.RULES) == 41 and not any("chroma_rows" in r.name for r in options.RULES)
    names = [r.name for r in options.RULES + options.FIELD_RULES + options.OUT_FIELD_RULES]
    assert len(set(names)) == len(names)

    def raw(hw=(36, 64), **kw):
        return options.Raw(render_hw=hw, **{n: kw.get(n, d) for n, d in defaults.items()})
    fired = set()
    cases = [("out_chroma_rows", dict(out_chroma_rows="both"), ("keywords",)), ("out_chroma_rows_format", dict(out_chroma_rows="interlaced"), ("keywords", "flags")),
             ("out_chroma_rows_height", dict(out_chroma_rows="interlaced", out_pix_fmt="nv12"), ()),
             ("out_chroma_rows_height", dict(out_chroma_rows="interlaced", out_pix_fmt="nv12", deliver_size=(40, 64)), ()),
             ("out_chroma_rows_height", dict(out_chroma_rows="interlaced", out_pix_fmt="nv12", deliver_size=(38, 64)), ("keywords", "flags"))]
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
    assert fired == {(r.name, s) for r in options.OUT_FIELD_RULES for s in ("keywords", "flags") if getattr(r, s) is not None}
    options.refuse(raw(hw=(None, 64), out_chroma_rows="interlaced", out_pix_fmt="nv12"), "flags", True)      # a height not given yet is not checked
    assert raw().out_chroma_rows == "progressive" and options.Raw(render_hw=(8, 8)).out_chroma_rows == "progressive"
    assert options.ChainOptions.out_chroma_rows == "progressive" and "out_chroma_rows" not in options.ChainOptions.__dataclass_fields__
    assert options.FieldChainOptions.__dataclass_fields__["out_chroma_rows"].default == "progressive"


# ---- the plans the ends build -------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def built(monkeypatch):
    """tests/test_chain_ends.py's recorders over every class an end may construct: (class, positional arguments, keywords)."""
    from pythoncrt_amd import adeint, canvas, deint, depth, field420, ingest, interlace, lut3d, resample, resize16, signal as signal_mod
    from tests.test_chain_ends import STAGES
    log = []
    others = [ingest.IngestResize, resize16.ResizeHalf, resample.Resample, signal_mod.Signal, deint.Deinterlace, adeint.AdaptiveDeinterlace, canvas.Canvas,
              depth.Widen, depth.Narrow, lut3d.Lut3D, interlace.Interlace]
    for cls in STAGES + [field420.UnpackField420, field420.EgressField420] + others:
        def init(self, *args, _cls=cls, **kw):
            log.append((_cls, args, kw))
            if issubclass(_cls, _stage.StagePlan):
                self.frame_bytes = _cls._frame_bytes(args[1][0], args[1][1], kw["layout"])
        monkeypatch.setattr(cls, "__init__", init)
    return log


def test_egress_plan_and_the_delivery_end(built, monkeypatch):
    import torch
    from pythoncrt_amd import depth, egress, ends, field420, formats, interlace, options, sited
    # formats.egress_plan: the seventh parameter
    for fmt in model.LAYOUTS:
        for chroma in model.CHROMAS:
            del built[:]
            plan = formats.egress_plan("dev", (8, 10), fmt, "bt709", "pc", chroma, "interlaced")
            assert type(plan) is field420.EgressField420
            assert built == [(field420.EgressField420, ("dev", (8, 10)), {"layout": fmt, "matrix": "bt709", "range": "pc", "chroma": chroma})]
            del built[:]
            assert type(formats.egress_plan("dev", (8, 10), fmt, "bt709", "pc", chroma, rows="progressive")) is not field420.EgressField420
            assert type(formats.egress_plan("dev", (8, 10), fmt, "bt709", "pc", chroma)) is type(formats.egress_plan("dev", (8, 10), fmt, "bt709", "pc", chroma, "progressive"))
    assert formats.egress_plan("dev", (8, 10), "rgb24", "bt601", "tv", "center", "interlaced") is None
    # DeliveryEnd: with the default, egress_plan is called with today's six positional arguments and nothing more
    calls = []
    real = formats.egress_plan
    monkeypatch.setattr(formats, "egress_plan", lambda *a, **kw: calls.append((a, kw)) or real(*a, **kw))
    del built[:]
    end = ends.DeliveryEnd("dev", (16, 20), torch.uint8, "nv12", "bt601", "tv", "left", None, "bilinear", interlace=("tff", "linear"))
    assert calls == [(("dev", (16, 20), "nv12", "bt601", "tv", "left"), {})]
    assert [b[0] for b in built] == [interlace.Interlace, sited.EgressSited] and end.frames(5) == 3
    del calls[:], built[:]
    end = ends.DeliveryEnd("dev", (16, 20), torch.uint8, "nv12", "bt601", "tv", "left", None, "bilinear", interlace=("tff", "linear"), chroma_rows="interlaced")
    assert calls == [(("dev", (16, 20), "nv12", "bt601", "tv", "left", "interlaced"), {})]
    assert [b[0] for b in built] == [interlace.Interlace, field420.EgressField420]
    assert built[1] == (field420.EgressField420, ("dev", (16, 20)), {"layout": "nv12", "matrix": "bt601", "range": "tv", "chroma": "left"})
    assert type(end.egress) is field420.EgressField420 and end.frame_bytes == 16 * 20 + 2 * 8 * 10 and end.shape(3) == (3, end.frame_bytes)
    del calls[:], built[:]
    end = ends.DeliveryEnd("dev", (16, 20), torch.float16, "yuv420p", "bt601", "tv", "center", (8, 12), "bilinear", narrow="ordered", chroma_rows="interlaced")
    assert calls == [(("dev", (8, 12), "yuv420p", "bt601", "tv", "center", "interlaced"), {})]         # built for the DELIVERY size, behind the Narrow
    assert [b[0] for b in built][-2:] == [depth.Narrow, field420.EgressField420] and end.frame_bytes == 8 * 12 + 2 * 4 * 6
    del calls[:], built[:]
    ends.DeliveryEnd("dev", (8, 10), torch.uint8, "yuv420p", "bt601", "tv", "center", None, "bilinear", chroma_rows="progressive")
    assert calls == [(("dev", (8, 10), "yuv420p", "bt601", "tv", "center"), {})] and [b[0] for b in built] == [egress.EgressYuv]
    # ChainOptions: the keyword is passed on only where it is not the default
    seen, sources = [], []
    monkeypatch.setattr(ends, "DeliveryEnd", lambda *a, **kw: seen.append((a, kw)))
    monkeypatch.setattr(ends, "SourceEnd", lambda *a, **kw: sources.append((a, kw)))
    defaults = _defaults()

    def spec(**kw):
        v = options.Raw(render_hw=(8, 10), **{n: kw.get(n, d) for n, d in defaults.items()})
        return options.ChainOptions.build(v, "keywords")
    a, b = spec(out_pix_fmt="nv12"), spec(out_pix_fmt="nv12", out_chroma_rows="interlaced", out_chroma="left")
    assert a.out_chroma_rows == "progressive" and type(a) is options.ChainOptions
    assert b.out_chroma_rows == "interlaced" and b.in_chroma_rows == "progressive" and type(b) is options.FieldChainOptions
    assert a != b
    a.delivery_end("dev", torch.uint8)
    b.delivery_end("dev", torch.uint8)
    assert "chroma_rows" not in seen[0][1] and seen[1][1]["chroma_rows"] == "interlaced" and seen[1][0][6] == "left"
    assert {k: v for k, v in seen[1][1].items() if k != "chroma_rows"} == seen[0][1] and seen[1][0][:6] == seen[0][0][:6]
    b.source_end("dev", (8, 10), torch.uint8)
    assert "chroma_rows" not in sources[0][1]
    # both *_chroma_rows keywords together, and the source one alone
    del seen[:], sources[:]
    c = spec(in_pix_fmt="nv12", out_pix_fmt="nv12", in_chroma_rows="interlaced", out_chroma_rows="interlaced", deinterlace="linear", deinterlace_fields="both",
             deliver_interlace="tff")
    d = spec(in_pix_fmt="nv12", out_pix_fmt="nv12", in_chroma_rows="interlaced")
    assert (c.in_chroma_rows, c.out_chroma_rows, d.in_chroma_rows, d.out_chroma_rows) == ("interlaced", "interlaced", "interlaced", "progressive")
    assert type(c) is type(d) is options.FieldChainOptions and c.weave == ("tff", "none")
    for s in (c, d):
        s.source_end("dev", (8, 10), torch.uint8)
        s.delivery_end("dev", torch.uint8)
    assert sources[0][1]["chroma_rows"] == sources[1][1]["chroma_rows"] == "interlaced"
    assert seen[0][1]["chroma_rows"] == "interlaced" and seen[0][1]["interlace"] == ("tff", "none") and "chroma_rows" not in seen[1][1]


# ---- the kernel builds ----------------------------------------------------------------------------------------------------------------------------

def test_the_eight_kernel_builds_and_their_registers():
    """Exactly eight builds (four layouts x two paths) in crtfx_egress_field420_impl, read from the library's code objects
    (tools/kernel_resources.py): no spills, no scratch, no LDS, no AGPRs, at most 128 registers — and the VGPR counts the header states."""
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n: v for n, v in res.items() if n.startswith("crtfx_egress_field420_impl::")}
    assert set(found) == {f"crtfx_egress_field420_impl::k_egress_field420<{l}, {p}>" for l in range(4) for p in (0, 1)}, sorted(found)
    text = open(HEADER).read()
    stated = {name: (int(v), int(g)) for name, v, g in re.findall(r"(\w+) (\d+) / (\d+)", text[text.index("Registers (gfx950"):text.index("no AGPRs")])}
    assert list(stated) == list(model.LAYOUTS), stated
    for name, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == 0 and v["agpr_count"] == 0 and v["vgpr_count"] + v["agpr_count"] <= 128, (name, v)
        layout, path = map(int, re.search(r"<(\d), (\d)>", name).groups())
        assert v["vgpr_count"] == stated[model.LAYOUTS[layout]][1 - path], (name, v["vgpr_count"], stated)
