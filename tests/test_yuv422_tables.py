"""The 8-bit 4:2:2 pair without a GPU: the layouts and their helpers, the ties of tests/yuv422_model.py to the 4:2:0 models that are already
trusted, the integer models against their float64 restatements, the odd-width pad byte, the C-ABI of include/crtfx_422.h bound symbol for
symbol and failing cleanly without a device, the twelve kernel builds' registers, and the refusals of process_frames and the CLI that need
no device."""
import ctypes
import io
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pythoncrt_amd import _lib, tables  # noqa: E402
from tests import unpack_model, yuv_model  # noqa: E402
from tests import yuv422_model as model  # noqa: E402

SIZES = [(1, 1), (2, 2), (3, 5), (16, 64), (37, 131), (1080, 1920)]


# ---- layout -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", model.LAYOUTS)
@pytest.mark.parametrize("h,w", SIZES)
def test_frame_bytes_offsets_and_split_planes(h, w, layout):
    from pythoncrt_amd import yuv422
    cw, fb = model.sizes(h, w, layout)
    assert cw == -(-w // 2)
    assert yuv422.frame_bytes(h, w, layout) == fb == (h * w + 2 * h * cw if layout == "yuv422p" else 4 * h * cw)
    if w % 2 == 0:
        assert fb == 2 * h * w                                                 # the formats' definition: 2 bytes per pixel
    p = np.arange(fb, dtype=np.uint32).astype(np.uint8) if h * w > 10000 else model.sources(h, w, layout, n=1)[0]
    y, u, v = yuv422.split_planes(p, (h, w), layout)
    assert y.shape == (h, w) and u.shape == v.shape == (h, cw) and all(np.shares_memory(t, p) for t in (y, u, v))
    my, mu, mv = model.planes(p, h, w, layout)
    assert np.array_equal(y, my) and np.array_equal(u, mu) and np.array_equal(v, mv)
    # byte offsets, written out
    for yy, xx in ((0, 0), (h - 1, 0), (0, w - 1), (h // 2, w // 2), (h - 1, w - 1)):
        cx = xx >> 1
        if layout == "yuv422p":
            oy, ou, ov = yy * w + xx, h * w + yy * cw + cx, h * w + h * cw + yy * cw + cx
        else:
            base = (yy * cw + cx) * 4
            y0, y1, pu, pv = (0, 2, 1, 3) if layout == "yuyv422" else (1, 3, 0, 2)
            oy, ou, ov = base + (y1 if xx & 1 else y0), base + pu, base + pv
        assert (y[yy, xx], u[yy, cx], v[yy, cx]) == (p[oy], p[ou], p[ov])
    # split_planes round-trips: the planes packed again are the frame (an odd width's pad byte aside, which the views leave out)
    back = model.pack_planes(np.ascontiguousarray(y), np.ascontiguousarray(u), np.ascontiguousarray(v), layout)
    if w % 2 and layout != "yuv422p":
        pad = np.zeros(fb, dtype=bool)
        pad.reshape(h, cw, 4)[:, -1, 2 if layout == "yuyv422" else 3] = True
        assert np.array_equal(back[~pad], p[~pad]) and np.array_equal(back[pad], y[:, -1])
    else:
        assert np.array_equal(back, p)
    # a batch, numpy and torch
    import torch
    if h * w <= 10000:
        batch = np.stack([p, p[::-1]])
        by, bu, bv = yuv422.split_planes(torch.from_numpy(batch), (h, w), layout)
        assert tuple(by.shape) == (2, h, w) and tuple(bu.shape) == tuple(bv.shape) == (2, h, cw)
        assert np.array_equal(by[0].numpy(), y) and np.array_equal(bu[0].numpy(), u) and np.array_equal(bv[0].numpy(), v)
        ry, ru, rv = model.planes(batch[1], h, w, layout)
        assert np.array_equal(by[1].numpy(), ry) and np.array_equal(bv[1].numpy(), rv)
    with pytest.raises(ValueError):
        yuv422.split_planes(p[:-1], (h, w), layout)
    with pytest.raises(ValueError):
        yuv422.split_planes(p, (h, w), "nv12")
    with pytest.raises(ValueError):
        yuv422.frame_bytes(h, w, "yuv420p")


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (16, 64), (37, 131)])
def test_the_three_layouts_carry_the_same_samples(h, w):
    from pythoncrt_amd import yuv422
    rgb = model.frames(h, w, n=1)[0]
    ref = model.convert(rgb)
    for layout in model.LAYOUTS:
        p = model.pack(rgb, layout)
        for got, exp in zip(yuv422.split_planes(p, (h, w), layout), ref):
            assert np.array_equal(got, exp), layout
        for other in model.LAYOUTS:
            assert np.array_equal(model.relayout(p, h, w, layout, other), model.pack(rgb, other))
        assert np.array_equal(model.unpack(p, h, w, layout), model.unpack(model.pack(rgb, "yuv422p"), h, w, "yuv422p"))


@pytest.mark.parametrize("layout", ("yuyv422", "uyvy422"))
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (37, 131)])
def test_odd_width_pad_byte(h, w, layout):
    """Written: a copy of the row's last Y.  Read: ignored — randomise it and the RGB does not move."""
    cw, fb = model.sizes(h, w, layout)
    rgb = model.frames(h, w, n=1)[0]
    p = model.pack(rgb, layout)
    pos = 2 if layout == "yuyv422" else 3
    y = model.convert(rgb)[0]
    assert np.array_equal(p.reshape(h, cw, 4)[:, -1, pos], y[:, -1])
    ref = model.unpack(p, h, w, layout)
    q = p.copy()
    q.reshape(h, cw, 4)[:, -1, pos] = np.random.default_rng(3).integers(0, 256, h, dtype=np.uint8)
    assert not np.array_equal(q, p) and np.array_equal(model.unpack(q, h, w, layout), ref)


def test_iter_yuv422_reads_frames():
    import pythoncrt_amd as pc
    from pythoncrt_amd import yuv422
    h, w = 5, 7

    class Dribble(io.BytesIO):                                  # a pipe may return less than asked for
        def read(self, n=-1):
            return super().read(min(n, 11) if n and n > 0 else n)
    for layout in model.LAYOUTS:
        fb = yuv422.frame_bytes(h, w, layout)
        data = np.random.default_rng(4).integers(0, 256, 3 * fb + fb // 2, dtype=np.uint8)
        for stream in (io.BytesIO(data.tobytes()), Dribble(data.tobytes())):
            got = list(pc.iter_yuv422(stream, w, h, layout))
            assert len(got) == 3 and all(f.shape == (fb,) and f.dtype == np.uint8 for f in got)
            assert np.array_equal(np.concatenate(got), data[:3 * fb])
    with pytest.raises(ValueError):
        next(pc.iter_yuv422(io.BytesIO(b""), w, h, "nv12"))


# ---- ties to the 4:2:0 models -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_luma_is_the_420_stage_s(matrix, rng):
    for h, w in ((3, 5), (16, 64), (37, 131)):
        rgb = model.frames(h, w, n=1)[0]
        assert np.array_equal(model.convert(rgb, matrix, rng)[0], yuv_model.convert(rgb, matrix, rng)[0])


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_unpack_with_pairwise_equal_chroma_rows_is_the_420_unpack(matrix, rng):
    """A 4:2:2 frame whose chroma rows 2 cy and 2 cy + 1 are equal holds a 4:2:0 frame: both models give the same RGB."""
    for h, w in ((2, 2), (3, 5), (16, 64), (37, 131)):
        ch, cw, fb420 = unpack_model.sizes(h, w)
        p420 = unpack_model.images(h, w)[0]
        y, u, v = unpack_model.planes(p420, h, w, "yuv420p")
        rows = np.arange(h) >> 1
        exp = unpack_model.unpack(p420, h, w, "yuv420p", matrix, rng)
        for layout in model.LAYOUTS:
            p422 = model.pack_planes(y, u[rows], v[rows], layout)
            assert np.array_equal(model.unpack(p422, h, w, layout, matrix, rng), exp), (h, w, layout)


def _uniform_pairs(cols):
    """1 x (2 n) x 3: every colour fills one horizontal pair."""
    return np.repeat(np.asarray(cols, dtype=np.uint8)[None, :, :], 2, axis=1)


def _lattice():
    steps = np.rint(np.linspace(0, 255, 33)).astype(np.uint8)
    assert len(set(steps.tolist())) == 33
    return np.stack(np.meshgrid(steps, steps, steps, indexing="ij"), axis=-1).reshape(-1, 3)


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_a_uniform_pair_has_the_per_pixel_chroma(matrix, rng):
    cols = np.concatenate([_lattice()[::7], np.array(yuv_model.CLAMP_COLOURS, dtype=np.uint8)])
    _, u, v = model.convert(_uniform_pairs(cols), matrix, rng)
    m, off = np.array(model.YUV_MATRICES[(matrix, rng)], dtype=np.int64), model.OFFSETS[rng]
    c = cols.astype(np.int64)
    for plane, row in ((u, 1), (v, 2)):
        assert np.array_equal(plane[0], np.clip((c @ m[row] + (off[row] << 16) + (1 << 15)) >> 16, 0, 255))
    # ... which is the 4:2:0 stage's chroma of the uniform 2 x 2 block
    block = np.repeat(_uniform_pairs(cols), 2, axis=0)
    _, u0, v0 = yuv_model.convert(block, matrix, rng)
    assert np.array_equal(u[0], u0[0]) and np.array_equal(v[0], v0[0])


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_greys(matrix, rng):
    """Egress: every grey gives U = V = 128.  Source: every grey (U = V = 128) gives R = G = B."""
    greys = [(g, g, g) for g in range(256)]
    y, u, v = model.convert(_uniform_pairs(greys), matrix, rng)
    assert (u == 128).all() and (v == 128).all()
    assert (int(y[0, 0]), int(y[0, -1])) == ((16, 235) if rng == "tv" else (0, 255))
    # mixed pairs of greys too: the chroma rows sum to 0
    mixed = np.array(greys, dtype=np.uint8)[None, np.random.default_rng(5).permutation(256)]
    _, u, v = model.convert(mixed, matrix, rng)
    assert (u == 128).all() and (v == 128).all()
    g = np.arange(256, dtype=np.uint8)[None, :]
    c = np.full((1, 128), 128, dtype=np.uint8)
    for layout in model.LAYOUTS:
        rgb = model.unpack(model.pack_planes(g, c, c, layout), 1, 256, layout, matrix, rng)
        assert np.array_equal(rgb[..., 0], rgb[..., 1]) and np.array_equal(rgb[..., 1], rgb[..., 2])
        assert (np.diff(rgb[0, :, 0].astype(int)) >= 0).all()


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_the_clamp_colours_hit_both_clamps(matrix, rng):
    """Source (the colours of test_unpack_tables.py): the accumulator passes 255 and falls below 0.  Egress (those of test_egress_tables.py):
    at full range pure blue's U and pure red's V are 256 before the clamp; the accumulators never fall below 0 (create's rule)."""
    m = np.array(model.RGB_MATRICES[(matrix, rng)], dtype=np.int64)
    off = np.array(model.OFFSETS[rng], dtype=np.int64)
    cols = np.array(unpack_model.CLAMP_COLOURS, dtype=np.int64)
    before = ((cols - off) @ m.T + (1 << 15)) >> 16
    assert before.max() > 255 and before.min() < 0
    yuv = cols.astype(np.uint8)
    y, c = np.repeat(yuv[None, :, 0], 2, axis=1), yuv[None, :, 1:]
    for layout in model.LAYOUTS:
        rgb = model.unpack(model.pack_planes(y, c[..., 0], c[..., 1], layout), 1, 2 * len(cols), layout, matrix, rng)
        assert np.array_equal(rgb[0, ::2].astype(np.int64), np.clip(before, 0, 255)) and np.array_equal(rgb[0, ::2], rgb[0, 1::2])
        assert rgb.max() == 255 and rgb.min() == 0
    if rng == "pc":
        me = np.array(model.YUV_MATRICES[(matrix, rng)], dtype=np.int64)
        for colour, row in (((0, 0, 255), 1), ((255, 0, 0), 2)):
            s = 2 * np.array(colour, dtype=np.int64)
            assert (s @ me[row] + (128 << 17) + (1 << 16)) >> 17 == 256
        _, u, v = model.convert(_uniform_pairs([(0, 0, 255), (255, 0, 0)]), matrix, rng)
        assert int(u[0, 0]) == 255 and int(v[0, 1]) == 255
    _, u, v = model.convert(_uniform_pairs(yuv_model.CLAMP_COLOURS), matrix, rng)        # asserts acc >= 0 inside
    assert u.min() < 128 < u.max() and v.min() < 128 < v.max()


# ---- the integer models against the float64 restatements ----------------------------------------------------------------------------------

BOUND = 3 * 255 * 2.0 ** -16            # tests/test_egress_tables.py: the most three coefficients rounded to 2^-16 (and the G adjustment) move a sum


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_egress_model_against_the_float_restatement(matrix, rng):
    """The 33-step lattice as uniform pairs and as mixed pairs (each colour beside its successor): Y, U, V are the float64 ones except where
    the float value lies within 3 * 255 * 2^-16 of a half-integer, and there they differ by one code.  A pair is a sum of two samples
    shifted by 17: the coefficient error per unit of the mean is the same, so the bound is."""
    lat = _lattice()
    for img in (_uniform_pairs(lat), np.stack([lat, np.roll(lat, -1, axis=0)], axis=1).reshape(1, -1, 3)):
        got = model.convert(img, matrix, rng)
        exp, raw = model.convert_float(img, matrix, rng)
        for g, e, r in zip(got, exp, raw):
            d = g.astype(np.int64) - e.astype(np.int64)
            assert np.abs(d).max() <= 1
            dist = np.abs(r - np.floor(r) - 0.5)
            assert (dist[d != 0] <= BOUND).all(), float(dist[d != 0].max())


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_source_model_against_the_float_restatement(matrix, rng):
    """The 33-step lattice of (Y, U, V): the same statement for the source direction (its three coefficients are rounded, none adjusted)."""
    lat = _lattice()
    y, u, v = np.repeat(lat[None, :, 0], 2, axis=1), lat[None, :, 1], lat[None, :, 2]
    for layout in model.LAYOUTS:
        p = model.pack_planes(y, u, v, layout)
        got = model.unpack(p, 1, 2 * len(lat), layout, matrix, rng)
        exp, raw = model.unpack_float(p, 1, 2 * len(lat), layout, matrix, rng)
        d = got.astype(np.int64) - exp.astype(np.int64)
        assert np.abs(d).max() <= 1
        dist = np.abs(raw - np.floor(raw) - 0.5)
        assert (dist[d != 0] <= BOUND).all(), float(dist[d != 0].max())


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------

FAMILIES = ("unpack422", "egress422")


def test_header_prototypes_are_the_bound_symbols():
    """include/crtfx_422.h declares exactly _lib.YUV422_SYMBOLS (argument counts included): two families of seven that mirror crtfx_unpack_* /
    crtfx_egress_* signature for signature; the table is disjoint from the others; both new files are sources of the build; the built library
    exports every symbol."""
    hdr = open(os.path.join(ROOT, "include", "crtfx_422.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_(?:unpack422|egress422)_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(_lib.YUV422_SYMBOLS) and len(protos) == 14, set(protos) ^ set(_lib.YUV422_SYMBOLS)
    others = set(_lib.SYMBOLS) | set(_lib.INGEST_SYMBOLS) | set(_lib.EGRESS_SYMBOLS) | set(_lib.UNPACK_SYMBOLS) | set(_lib.DEEP_SYMBOLS)
    assert not set(_lib.YUV422_SYMBOLS) & others
    for name, args in protos.items():
        n_args = 0 if args.strip() in ("", "void") else len(args.split(","))
        assert n_args == len(_lib.YUV422_SYMBOLS[name][1]), name
        assert _lib.YUV422_SYMBOLS[name] == _lib.UNPACK_SYMBOLS[name.replace("crtfx_unpack422_", "crtfx_unpack_").replace("crtfx_egress422_", "crtfx_unpack_")], name
    assert re.search(r"CRTFX_422_YUV422P\s*=\s*0\s*,\s*CRTFX_422_YUYV422\s*=\s*1\s*,\s*CRTFX_422_UYVY422\s*=\s*2", hdr)
    assert (_lib.YUV422_YUV422P, _lib.YUV422_YUYV422, _lib.YUV422_UYVY422, _lib.UNPACK422_OPT_FORCE_GENERAL, _lib.EGRESS422_OPT_FORCE_GENERAL) == (0, 1, 2, 1, 1)
    assert all(os.path.basename(f) in {os.path.basename(s) for s in _lib.SOURCES} for f in ("crtfx_422.hip", "crtfx_422.h"))
    lib = _lib.load()
    for name in _lib.YUV422_SYMBOLS:
        assert getattr(lib, name).argtypes == _lib.YUV422_SYMBOLS[name][1]
    import pythoncrt_amd as pc
    assert all(n in pc.__all__ for n in (pc.UnpackYuv422.__name__, pc.EgressYuv422.__name__, pc.iter_yuv422.__name__))


def _table(fam):
    return tables.rgb_matrix if fam == "unpack422" else tables.yuv_matrix


def _create(lib, fam, h=12, w=20, pix_fmt=_lib.PIX_U8, layout=_lib.YUV422_UYVY422, device=0, m=None, off=None, null=False, null_off=False):
    tm, toff = _table(fam)("bt601", "tv")
    m = tm if m is None else np.ascontiguousarray(m, dtype=np.int32)
    off = toff if off is None else np.ascontiguousarray(off, dtype=np.int32)
    plan = ctypes.c_void_p(1)
    rc = getattr(lib, f"crtfx_{fam}_create")(device, h, w, pix_fmt, layout, None if null else tables.ptr(m), None if null_off else tables.ptr(off),
                                                 ctypes.byref(plan))
    return rc, plan, (getattr(lib, f"crtfx_{fam}_last_error")(None) or b"").decode()


@pytest.mark.parametrize("fam", FAMILIES)
def test_create_refuses_bad_arguments_before_it_touches_a_device(fam):
    """The argument checks come first, so they hold on any machine: half frames are UNSUPPORTED and the message names uint8; a size < 1 or
    > 32767, layout 3, an unknown pixel format, a null table, an offset outside 0..255 and a matrix whose accumulator could leave its
    range are INVALID; each leaves *out_plan NULL and a message.  A matrix that just fits is admitted."""
    lib = _lib.load()
    good = _table(fam)("bt601", "tv")[0]
    too_big, too_negative, fits = good.copy(), good.copy(), good.copy()
    if fam == "unpack422":
        too_big[0] = 1 << 23                                  # R row: 255 * 2^23 passes 2^31
        too_negative[4] = -(1 << 23)                          # G row: the rule sums magnitudes
        fits[0:3] = (8421375, 0, 0)                           # 255 * 8421375 + 2^15 = 2^31 - 255: admitted (8421376 is not)
        assert 255 * 8421375 + (1 << 15) == 2 ** 31 - 255 and 255 * 8421376 + (1 << 15) >= 2 ** 31
    else:
        too_big[0] = 1 << 23                                  # Y row: 255 * 2^23 passes 2^31
        too_negative[4] = -40000                              # U row: 2^24 + 2^16 - 510 * (9714 + 40000) < 0
        fits[0:3] = (8417263, 0, 0)                           # 255 * 8417263 + 16 * 2^16 + 2^15 = 2^31 - 239: admitted (8417264 is not)
        assert 255 * 8417263 + (16 << 16) + (1 << 15) == 2 ** 31 - 239 and 255 * 8417264 + (16 << 16) + (1 << 15) >= 2 ** 31
        assert (128 << 17) + (1 << 16) - 510 * (9714 + 40000) < 0
    over = fits.copy()
    over[0] += 1
    cases = [(dict(m=over), _lib.E_INVALID, "accumulator"), (dict(pix_fmt=_lib.PIX_F16), _lib.E_UNSUPPORTED, "uint8"), (dict(h=0), _lib.E_INVALID, "size"),
             (dict(w=0), _lib.E_INVALID, "size"), (dict(w=32768), _lib.E_INVALID, "size"), (dict(h=32768), _lib.E_INVALID, "size"),
             (dict(null=True), _lib.E_INVALID, "null"), (dict(null_off=True), _lib.E_INVALID, "null"), (dict(null=True, null_off=True), _lib.E_INVALID, "null"),
             (dict(pix_fmt=7), _lib.E_INVALID, "pixel format"), (dict(layout=3), _lib.E_INVALID, "layout"),
             (dict(layout=-1), _lib.E_INVALID, "layout"), (dict(off=(16, 256, 128)), _lib.E_INVALID, "offset"), (dict(off=(-1, 128, 128)), _lib.E_INVALID, "offset"),
             (dict(m=too_big), _lib.E_INVALID, "accumulator"), (dict(m=too_negative), _lib.E_INVALID, "accumulator")]
    for kw, code, word in cases:
        rc, plan, msg = _create(lib, fam, **kw)
        assert rc == code and not plan.value and word in msg, (kw, rc, plan.value, msg)
    for kw in (dict(m=fits), dict(h=32767, w=32767), dict(layout=0), dict(layout=1)):
        rc, plan, msg = _create(lib, fam, **kw)
        assert rc in (_lib.OK, _lib.E_HIP), (kw, rc, msg)         # no device here: E_HIP; with one: a plan
        if rc == _lib.OK:
            assert getattr(lib, f"crtfx_{fam}_destroy")(plan) == _lib.OK
    f = lambda name: getattr(lib, f"crtfx_{fam}_{name}")          # noqa: E731
    assert f("destroy")(None) == _lib.OK and f("set_option")(None, 1, 1) == _lib.E_INVALID
    assert f("run")(None, None, 0, None, 0, 1, None) == _lib.E_INVALID and f("frame_bytes")(None) == 0
    assert f("last_plan")(None, ctypes.create_string_buffer(8), 8) == _lib.E_INVALID


@pytest.mark.parametrize("fam", FAMILIES)
def test_create_without_a_gpu_fails_cleanly(fam):
    import torch
    lib = _lib.load()
    if torch.cuda.is_available():
        rc, plan, msg = _create(lib, fam, device=4096)          # no such device on any box
        assert rc == _lib.E_HIP and not plan.value and "4096" in msg
        return
    rc, plan, msg = _create(lib, fam)
    assert rc == _lib.E_HIP and not plan.value and msg, (rc, msg)


def test_the_420_entry_points_still_refuse_layout_2():
    """The new formats have entry points of their own: crtfx_unpack_create / crtfx_egress_create answer layout 2 as they did."""
    lib = _lib.load()
    for fam, table in (("unpack", tables.rgb_matrix), ("egress", tables.yuv_matrix)):
        m, off = table("bt601", "tv")
        plan = ctypes.c_void_p(1)
        rc = getattr(lib, f"crtfx_{fam}_create")(0, 12, 20, _lib.PIX_U8, 2, tables.ptr(m), tables.ptr(off), ctypes.byref(plan))
        assert rc == _lib.E_INVALID and not plan.value


def test_the_twelve_kernel_builds_and_their_registers():
    """Exactly twelve kernel builds (two directions x three layouts x two paths) in the library's code objects (tools/kernel_resources.py):
    no spills, no scratch memory, no LDS, and at most 64 VGPRs + AGPRs — the bar of the 8-bit 4:2:0 stages."""
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n: v for n, v in res.items() if n.startswith("crtfx_422_impl::")}
    assert set(found) == {f"crtfx_422_impl::k_{d}_422<{l}, {p}>" for d in ("unpack", "egress") for l in (0, 1, 2) for p in (0, 1)}, sorted(found)
    for name, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == 0 and v["vgpr_count"] + v["agpr_count"] <= 64, (name, v)


# ---- refusals that need no device -----------------------------------------------------------------------------------------------------------

def test_process_frames_refuses_before_it_touches_a_device():
    """A 4:2:2 format opposite a 10-bit one is the "one end" ValueError; resize_on="host" with a 4:2:2 input is refused as for nv12; an
    unknown name is still refused with the text the 4:2:0 tests match; no frame is read and nothing is written."""
    import pythoncrt_amd as pc

    def never():
        raise AssertionError("a frame was read")
        yield

    def call(**kw):
        return pc.process_frames(never(), lambda a: (_ for _ in ()).throw(AssertionError("written")), 64, 36, 30.0, 1, **kw)
    for kw, word in ((dict(in_pix_fmt="uyvy422", out_pix_fmt="p010le"), "one end"), (dict(in_pix_fmt="yuv420p10le", out_pix_fmt="yuv422p"), "one end"),
                     (dict(in_pix_fmt="p010le", out_pix_fmt="yuyv422"), "one end"),
                     (dict(in_pix_fmt="uyvy422", resize_on="host"), "host"), (dict(in_pix_fmt="yuv422p", out_pix_fmt="yuyv422", resize_on="host"), "host"),
                     (dict(in_pix_fmt="yuv444p"), "in_pix_fmt must be 'rgb24', 'yuv420p' or 'nv12'"),
                     (dict(out_pix_fmt="yuv422p10le"), "out_pix_fmt must be 'rgb24', 'yuv420p' or 'nv12'"),
                     (dict(in_pix_fmt="v210", out_pix_fmt="uyvy422"), "in_pix_fmt must be 'rgb24', 'yuv420p' or 'nv12'")):
        with pytest.raises(ValueError) as e:
            call(**kw)
        assert word in str(e.value), (kw, str(e.value))
    with pytest.raises(ValueError) as e:
        call(in_pix_fmt="yuv444p")
    assert all(n in str(e.value) for n in ("'yuv422p'", "'yuyv422'", "'uyvy422'"))           # the new names are appended to the message


def test_cli_refuses_before_it_touches_a_device(monkeypatch, tmp_path, capsys):
    """One end only: SystemExit that names both flags.  The sharded CLI refuses the 4:2:2 formats with the message form it uses for nv12:
    the flag with its value and the word "sharded".  The parser takes the three names and still rejects an unknown one."""
    from pythoncrt_amd import cli
    src = tmp_path / "in.yuv"
    src.write_bytes(bytes(8 * 8 * 3))
    base = ["--input", str(src), "--output", str(tmp_path / "out.yuv"), "--width", "8", "--height", "8"]
    for extra in (["--in-pix-fmt", "uyvy422", "--out-pix-fmt", "p010le"], ["--in-pix-fmt", "yuv420p10le", "--out-pix-fmt", "yuv422p"]):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code not in (0, None) and "one end" in str(e.value) and "--in-pix-fmt" in str(e.value) and "--out-pix-fmt" in str(e.value)
        assert not (tmp_path / "out.yuv").exists()
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    for name in model.LAYOUTS:
        for flag in ("--in-pix-fmt", "--out-pix-fmt"):
            with pytest.raises(SystemExit) as e:
                cli.main(base + [flag, name])
            assert f"{flag} {name}" in str(e.value) and "sharded" in str(e.value) and not (tmp_path / "out.yuv").exists()
    monkeypatch.delenv("WORLD_SIZE")
    parser = cli.add_input_flags(cli.add_output_flags(cli.build_parser()))
    for name in model.LAYOUTS:
        a = parser.parse_args(["--input", "x", "--in-pix-fmt", name, "--out-pix-fmt", name, "--in-matrix", "bt709", "--in-range", "pc",
                               "--out-matrix", "bt709", "--out-range", "pc"])
        assert (a.in_pix_fmt, a.out_pix_fmt, a.in_matrix, a.in_range, a.out_matrix, a.out_range) == (name, name, "bt709", "pc", "bt709", "pc")
        assert name in cli.IN_PIX_FMTS and name in cli.OUT_PIX_FMTS
    for flag in ("--in-pix-fmt", "--out-pix-fmt"):
        with pytest.raises(SystemExit) as e:
            parser.parse_args(["--input", "x", flag, "yuv444p"])
        assert e.value.code == 2
    capsys.readouterr()
