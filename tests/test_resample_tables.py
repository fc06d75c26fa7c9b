"""The filtered resampler without a GPU (include/crtfx_resample.h): the signed tables of tables.pil_filter_axis are pil_resample_axis's for
"bilinear"; the int64 model (tests/resample_model.py) equals the installed Pillow byte for byte under all five filters and drives both
clamps; the facts the kernels' accumulators rest on hold for every table tried; the half model is tied to the half BILINEAR model, to the
8-bit pass, to the two-accumulator identity of the kernels and to a float64 restatement; the C-ABI is bound symbol for symbol and refuses
bad arguments before it touches a device, as do Resample, process_frames(in_filter= / deliver_filter=) and both CLIs; the two BILINEAR
stages still refuse a negative coefficient; the builds' registers are the header's."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pythoncrt_amd import _lib, tables  # noqa: E402
from tests import pil_resize_model, resize16_model  # noqa: E402
from tests import resample_model as model  # noqa: E402

ALL_PAIRS = pil_resize_model.PAIRS + pil_resize_model.EXTRA_PAIRS
PAIR_AXES = sorted({(s[i], d[i]) for s, d in pil_resize_model.PAIRS for i in (0, 1)})
FACT_AXES = sorted(set(model.SPEC_AXES) | set(resize16_model.FULL_AXES))
SIGNED = ("bicubic", "lanczos")            # the filters with negative lobes


def _ids(s):
    return f"{s[0]}x{s[1]}"


def test_the_five_names_and_an_unknown_one():
    assert tables.RESAMPLE_FILTERS == ("box", "bilinear", "hamming", "bicubic", "lanczos")
    for bad in ("nearest", "LANCZOS", "", None, 3):
        with pytest.raises(ValueError, match="filter"):
            tables.pil_filter_axis(8, 4, bad)
    for n_in, n_out in ((0, 4), (4, 0)):
        with pytest.raises(ValueError):
            tables.pil_filter_axis(n_in, n_out, "lanczos")


@pytest.mark.parametrize("n_in,n_out", sorted(set(PAIR_AXES) | set(resize16_model.FULL_AXES)), ids=str)
def test_bilinear_tables_are_the_existing_ones(n_in, n_out):
    """pil_filter_axis(.., "bilinear") == pil_resample_axis array for array (values, shapes and dtypes): the signed builder restates the
    unsigned one, which stays untouched."""
    a, b = tables.pil_filter_axis(n_in, n_out, "bilinear"), tables.pil_resample_axis(n_in, n_out)
    for u, v in zip(a, b):
        assert u.dtype == v.dtype == np.int32 and u.shape == v.shape and np.array_equal(u, v) and u.flags.c_contiguous


@pytest.mark.parametrize("src,dst", ALL_PAIRS, ids=_ids)
@pytest.mark.parametrize("filter", model.FILTERS)
def test_the_8_bit_model_is_pillow(filter, src, dst):
    """resize_u8 == Image.resize((w, h), filter) of the installed Pillow: 0 bytes differ, five filters x every pair x both images."""
    for name, img in pil_resize_model.images(*src).items():
        got, exp = model.resize_u8(img, dst[0], dst[1], filter), model.pillow(img, dst[0], dst[1], filter)
        assert got.shape == exp.shape and got.dtype == np.uint8
        assert int((got != exp).sum()) == 0, (filter, src, dst, name, int((got != exp).sum()))


def test_the_blockwise_sums_are_the_plain_int64_sums():
    """resample_model.pass_sums (blocks of dense products, exact integers carried in float64) == the gather-multiply-add in int64, on uint8
    values and on quarter codes at the extremes, under every filter."""
    rng = np.random.default_rng(5)
    for src_n, dst_n in ((64, 128), (131, 41), (640, 16), (213, 214), (300, 2), (5, 1)):
        for top in (255, model.QMAX):
            img = rng.integers(0, top + 1, (7, src_n, 3), dtype=np.int64)
            img[0], img[1] = top, (np.arange(src_n) % 2 * top)[:, None]
            for filter in model.FILTERS:
                xmin, count, k = tables.pil_filter_axis(src_n, dst_n, filter)
                t = np.arange(k.shape[1])[None, :]
                idx = np.minimum(xmin[:, None] + t, src_n - 1)
                plain = (1 << 21) + np.einsum("rxtc,xt->rxc", img[:, idx, :], model.masked(count, k))
                got = model.pass_sums(img, xmin, count, k)
                assert got.dtype == np.int64 and np.array_equal(got, plain), (src_n, dst_n, top, filter)


@pytest.mark.parametrize("filter", SIGNED)
def test_the_binary_images_drive_both_clamps(filter):
    """Under bicubic and Lanczos the full-scale steps of the "binary" images push a sum below 0 AND above top, in the horizontal pass and in
    the vertical one, on uint8 values and on quarter codes: a kernel that clamps on one side only cannot give the model's bytes."""
    for src, dst in (((48, 64), (96, 128)), ((108, 192), (54, 96)), ((37, 61), (53, 85))):
        for top, img in ((255, pil_resize_model.images(*src)["binary"].astype(np.int64)),
                         (model.QMAX, resize16_model.quantise(resize16_model.images(*src)["binary"]))):
            ax, ay = tables.pil_filter_axis(src[1], dst[1], filter), tables.pil_filter_axis(src[0], dst[0], filter)
            pre_h = model.pass_sums(img, *ax) >> model.PREC
            assert pre_h.min() < 0 and pre_h.max() > top, (filter, src, dst, top, int(pre_h.min()), int(pre_h.max()))
            hor = np.clip(pre_h, 0, top)
            pre_v = model.pass_sums(np.ascontiguousarray(hor.transpose(1, 0, 2)), *ay) >> model.PREC
            assert pre_v.min() < 0 and pre_v.max() > top, (filter, src, dst, top, int(pre_v.min()), int(pre_v.max()))
    for name in ("box", "bilinear", "hamming"):          # non-negative taps that sum to 2^22 within their rounding: only a unit of overshoot
        img = pil_resize_model.images(48, 64)["binary"].astype(np.int64)
        pre = model.pass_sums(img, *tables.pil_filter_axis(64, 128, name)) >> model.PREC
        assert pre.min() >= 0 and pre.max() <= 256, name


@pytest.mark.parametrize("n_in,n_out", FACT_AXES, ids=str)
@pytest.mark.parametrize("filter", model.FILTERS)
def test_table_facts_the_kernels_rest_on(filter, n_in, n_out):
    """What crtfx_resample_create checks, on the axes the stage was specified with and on the full-size axes of the half resampler: windows
    inside the source and monotone, every coefficient a signed 24-bit operand, every partial sum of a top = 255 pass inside int32; negative
    taps exist for exactly bicubic and Lanczos."""
    xmin, count, k = tables.pil_filter_axis(n_in, n_out, filter)
    assert xmin.shape == count.shape == (n_out,) and k.shape[0] == n_out and k.dtype == np.int32
    assert xmin.min() >= 0 and count.min() >= 1 and count.max() <= k.shape[1] and (xmin + count).max() <= n_in
    assert (np.diff(xmin) >= 0).all() and (np.diff(xmin + count) >= 0).all()
    kk = model.masked(count, k)
    assert -(1 << 23) <= kk.min() and kk.max() < (1 << 23)
    pos, neg = np.where(kk > 0, kk, 0).sum(axis=1), np.where(kk < 0, kk, 0).sum(axis=1)
    assert (1 << 21) + 255 * int(pos.max()) < 2 ** 31 and 255 * int(neg.min()) > -2 ** 31
    assert np.abs(kk.sum(axis=1) - (1 << 22)).max() <= k.shape[1]                 # a row sums to 2^22 within a unit per tap
    if filter not in SIGNED:
        assert kk.min() >= 0
    elif (n_in, n_out) in model.SPEC_AXES:                                          # (a 32767 -> 1 window is clipped to the centre lobe: no negative tap)
        assert kk.min() < 0


@pytest.mark.parametrize("filter,pos_max,neg_max", [("bicubic", 1.1250, 0.1250), ("lanczos", 1.2717, 0.2717)])
def test_the_quarter_code_sum_needs_more_than_32_bits(filter, pos_max, neg_max):
    """The figures the header quotes, over the axes the stage was specified with: the positive taps of a row sum to at most 1.1250 x 2^22
    (bicubic) / 1.2717 x 2^22 (Lanczos), the negative ones to 0.1250 / 0.2717 — and with top = 1020 the sum of such a row leaves 32 bits,
    signed AND unsigned, which is why the half kernels do not accumulate as the uint8 ones do."""
    worst_pos = worst_neg = 0
    for n_in, n_out in model.SPEC_AXES:
        xmin, count, k = tables.pil_filter_axis(n_in, n_out, filter)
        kk = model.masked(count, k)
        worst_pos = max(worst_pos, int(np.where(kk > 0, kk, 0).sum(axis=1).max()))
        worst_neg = max(worst_neg, int(-np.where(kk < 0, kk, 0).sum(axis=1).min()))
    assert round(worst_pos / 2 ** 22, 4) == pos_max and round(worst_neg / 2 ** 22, 4) == neg_max, (worst_pos / 2 ** 22, worst_neg / 2 ** 22)
    assert (1 << 21) + model.QMAX * worst_pos >= 2 ** 32
    for n_in, n_out in ((3840, 1920), (1920, 3840)):                              # ... and at the sizes people deliver, each on its own
        xmin, count, k = tables.pil_filter_axis(n_in, n_out, filter)
        assert (1 << 21) + model.QMAX * int(np.where(k > 0, k, 0).astype(np.int64).sum(axis=1).max()) >= 2 ** 32


@pytest.mark.parametrize("filter", model.FILTERS)
def test_an_unchanged_axis_has_identity_tables(filter):
    """n -> n under every filter: one coefficient of 2^22 on the sample itself and zeros around it (the sinc's zeros round to 0), so the pass
    Pillow skips can be run: it returns its input."""
    for n in (1, 2, 7, 40, 1080, 3840):
        xmin, count, k = tables.pil_filter_axis(n, n, filter)
        kk = model.masked(count, k)
        idx = np.arange(n)
        assert ((xmin <= idx) & (idx < xmin + count)).all()
        assert (kk[idx, idx - xmin] == 1 << 22).all() and (kk != 0).sum() == n, (filter, n)
    img = pil_resize_model.images(30, 40)["random"]
    assert np.array_equal(model.resample_pass(img, *tables.pil_filter_axis(40, 40, filter)), img)


def test_the_half_model_with_bilinear_is_the_half_bilinear_model():
    for src, dst in pil_resize_model.PAIRS[:6] + pil_resize_model.EXTRA_PAIRS[1:2]:
        for name, img in resize16_model.images(*src).items():
            got, exp = model.resize_half(img, dst[0], dst[1], "bilinear"), resize16_model.resize(img, *dst)
            assert got.dtype == np.float16 and np.array_equal(got.view(np.uint16), exp.view(np.uint16)), (src, dst, name)


def test_the_pass_with_top_255_is_the_8_bit_pass():
    """One `resample_pass` serves both scales: with top = 255 it is pil_resize_model's pass under the bilinear tables, and resize_codes(top=255)
    is the resize_u8 that is held to Pillow."""
    for src, dst in pil_resize_model.PAIRS[:4]:
        img = pil_resize_model.images(*src)["random"]
        ax = tables.pil_filter_axis(src[1], dst[1], "bilinear")
        assert np.array_equal(model.resample_pass(img, *ax, top=255), pil_resize_model.resample_pass(img, *ax))
        for filter in model.FILTERS:
            assert np.array_equal(model.resize_codes(img.astype(np.int64), dst[0], dst[1], filter, top=255), model.resize_u8(img, dst[0], dst[1], filter))


def test_two_int32_accumulators_give_the_int64_sum():
    """The identity the half kernels use: with A = sum k * (q >> 2) and B = sum k * (q & 3), (2^21 + 4 A + B) >> 22 — and the 32-bit form
    (A + ((B + 2^21) >> 2)) >> 20 — equal (2^21 + sum k * q) >> 22 with arithmetic shifts, and A, B stay inside int32 for every table the
    admission rule lets in.  Random codes and random signed tables at the rule's edge, and the real tables."""
    rng = np.random.default_rng(20)
    rows = []
    for _ in range(400):
        n = int(rng.integers(1, 40))
        top = min(1 << 23, (1 << 25) // n)                                       # rows whose sums reach the rule's edge; some are past it
        k = rng.integers(-top, top, n, dtype=np.int64)
        pos, neg = int(k[k > 0].sum()), int(k[k < 0].sum())
        if (1 << 21) + 255 * pos >= 2 ** 31 or 255 * neg <= -2 ** 31:
            continue
        rows.append(k)
    assert len(rows) > 50
    for filter in SIGNED:
        for axis in ((3840, 1920), (1080, 2160), (131, 41)):
            xmin, count, k = tables.pil_filter_axis(*axis, filter)
            rows.extend(model.masked(count, k)[:: max(1, len(k) // 40)])
    for k in rows:
        q = rng.integers(0, model.QMAX + 1, (64, len(k)), dtype=np.int64)
        q[0], q[1] = model.QMAX * (k > 0), model.QMAX * (k < 0)                # the extreme sums of the row
        exact = ((1 << 21) + (q * k).sum(axis=1)) >> 22
        A, B = np.cumsum(k * (q >> 2), axis=1), np.cumsum(k * (q & 3), axis=1)
        assert np.abs(A).max() < 2 ** 31 and np.abs(B).max() < 2 ** 31
        A, B = A[:, -1], B[:, -1]
        assert np.array_equal((4 * A + B + (1 << 21)) >> 22, exact)
        assert np.array_equal((A + ((B + (1 << 21)) >> 2)) >> 20, exact)


@pytest.mark.parametrize("src,dst", ALL_PAIRS, ids=_ids)
@pytest.mark.parametrize("filter", model.FILTERS)
def test_half_model_against_the_float_restatement(filter, src, dst):
    """The model's quarter codes against the separable float64 sum with the weights k / 2^22 that clamps to 0..1020 where the model does.
    The horizontal pass rounds once (at most 1/2, and the clamp does not stretch it); the vertical pass carries that through its weights,
    at most 1/2 * max_row sum |k_y| / 2^22, and rounds once more: bound = 1/2 + 1/2 * max sum |k_y| / 2^22 (+ 1e-6 for the float sums)."""
    xmin, count, ky = tables.pil_filter_axis(src[0], dst[0], filter)
    bound = 0.5 + 0.5 * float(np.abs(model.masked(count, ky)).sum(axis=1).max()) / 2 ** 22 + 1e-6
    assert bound < 1.3
    for name, img in resize16_model.images(*src).items():
        q = resize16_model.quantise(img)
        got, ref = model.resize_codes(q, dst[0], dst[1], filter), model.resize_float(q, dst[0], dst[1], filter)
        assert got.shape == ref.shape == (dst[0], dst[1], 3) and got.min() >= 0 and got.max() <= model.QMAX
        err = float(np.abs(got - ref).max())
        assert err <= bound, (filter, src, dst, name, err, bound)
        out = model.resize_half(img, dst[0], dst[1], filter)
        assert out.dtype == np.float16 and np.array_equal(out.astype(np.float64) * 4.0, got.astype(np.float64))


def test_tile_footprints_are_the_ones_the_stage_was_specified_with():
    """The LDS footprint formula of the header, restated in resample_model.fused_shape, on the sizes people deliver: (rows, cols, bytes) for
    uint8 / 2-byte samples; a quarter-size Lanczos on halves fits no shape (the general path)."""
    UHD, FHD, UHD8 = (2160, 3840), (1080, 1920), (4320, 7680)
    for filter, src, dst, u8, half in (("lanczos", UHD, FHD, (16, 64, 30672), (8, 64, 36040)), ("lanczos", UHD8, UHD, (16, 64, 30672), (8, 64, 36040)),
                                       ("lanczos", FHD, UHD, (32, 128, 19048), (32, 128, 32072)), ("lanczos", UHD, (720, 1280), (8, 64, 38028), (8, 32, 37212)),
                                       ("lanczos", UHD, (540, 960), (8, 32, 32816), None), ("bicubic", UHD, FHD, (16, 64, 26472), (8, 64, 29480))):
        assert model.fused_shape(src, dst, filter, 1) == u8 and model.fused_shape(src, dst, filter, 2) == half, (filter, src, dst)
    for src, dst in ((UHD8, UHD), (FHD, UHD), (UHD, (720, 1280)), (UHD, (540, 960))):
        assert model.fused_shape(src, dst, "bicubic", 1) and model.fused_shape(src, dst, "bicubic", 2)
    assert model.fused_shape((360, 640), (9, 16), "lanczos", 1) is None and model.fused_shape((360, 640), (9, 16), "lanczos", 2) is None


def test_header_prototypes_are_the_bound_symbols():
    """include/crtfx_resample.h declares exactly _lib.RESAMPLE_SYMBOLS (argument counts included), the shape of the ingest stage's table, and
    the built library exports every one; the unit is a stage unit of its own."""
    hdr = open(os.path.join(ROOT, "include", "crtfx_resample.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_resample_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(_lib.RESAMPLE_SYMBOLS) and len(protos) == 6, set(protos) ^ set(_lib.RESAMPLE_SYMBOLS)
    others = (set(_lib.SYMBOLS) | set(_lib.INGEST_SYMBOLS) | set(_lib.EGRESS_SYMBOLS) | set(_lib.UNPACK_SYMBOLS) | set(_lib.DEEP_SYMBOLS) | set(_lib.YUV422_SYMBOLS)
              | set(_lib.DEEP444_SYMBOLS) | set(_lib.SITED_SYMBOLS) | set(_lib.EGRESS_SITED_SYMBOLS) | set(_lib.RESIZE16_SYMBOLS))
    assert not set(_lib.RESAMPLE_SYMBOLS) & others
    for name, args in protos.items():
        n_args = 0 if args.strip() in ("", "void") else len(args.split(","))
        assert n_args == len(_lib.RESAMPLE_SYMBOLS[name][1]), name
        assert _lib.RESAMPLE_SYMBOLS[name] == _lib.INGEST_SYMBOLS[name.replace("crtfx_resample_", "crtfx_ingest_")], name
    assert all(os.path.basename(f) in {os.path.basename(s) for s in _lib.SOURCES} for f in ("crtfx_resample.hip", "crtfx_resample.h"))
    assert "crtfx_resample" in _lib.STAGE_UNITS and (_lib.RESAMPLE_OPT_FORCE_GENERAL, _lib.RESAMPLE_OPT_ACC64) == (1, 2)
    assert re.search(r"CRTFX_RESAMPLE_OPT_FORCE_GENERAL\s*=\s*1\b", hdr) and re.search(r"CRTFX_RESAMPLE_OPT_ACC64\s*=\s*2\b", hdr)
    lib = _lib.load()
    for name in _lib.RESAMPLE_SYMBOLS:
        assert getattr(lib, name).argtypes == _lib.RESAMPLE_SYMBOLS[name][1]
    import pythoncrt_amd as pc
    assert pc.Resample.__name__ in pc.__all__


def _create(lib, src, dst, pix_fmt=_lib.PIX_U8, device=0, mutate=None, null=False, no_out=False, filter="lanczos", family="resample"):
    build = (lambda a, b: tables.pil_filter_axis(a, b, filter)) if family == "resample" else tables.pil_resample_axis
    ax, ay = build(src[1], max(1, min(dst[1], 32767))), build(src[0], max(1, min(dst[0], 32767)))
    if mutate:
        mutate(ax, ay)
    plan = ctypes.c_void_p(1)
    rc = getattr(lib, f"crtfx_{family}_create")(device, src[0], src[1], dst[0], dst[1], pix_fmt, None if null else tables.ptr(ax[0]), tables.ptr(ax[1]),
                                                tables.ptr(ax[2]), ax[2].shape[1], tables.ptr(ay[0]), tables.ptr(ay[1]), tables.ptr(ay[2]), ay[2].shape[1],
                                                None if no_out else ctypes.byref(plan))
    return rc, plan, (getattr(lib, f"crtfx_{family}_last_error")(None) or b"").decode()


def test_create_refuses_bad_arguments_before_it_touches_a_device():
    """The argument checks of crtfx_resample_create come first, so they hold on any machine: an unknown pixel format, sizes 0 and 32768, a
    null table, a decreasing min, count > ksize, a coefficient outside the signed 24 bits on either side, a row whose positive or negative
    taps could carry a sum out of int32 and a null out pointer are INVALID, for uint8 and for half frames alike; each leaves *out_plan NULL
    and a message."""
    lib = _lib.load()

    def moves_back(ax, ay):
        ay[0][1] = ay[0][2] + 1

    def count_over_ksize(ax, ay):
        ax[1][3] = ax[2].shape[1] + 1

    def k_too_large(ax, ay):
        ax[2][5, 0] = 1 << 23

    def k_too_small(ax, ay):
        ay[2][5, 0] = -(1 << 23) - 1

    def positive_row_leaves_int32(ax, ay):
        ax[2][5, :3] = (1 << 23) - 1                 # 2^21 + 255 * 3 * (2^23 - 1) >= 2^31, each coefficient inside its 24 bits

    def negative_row_leaves_int32(ax, ay):
        ay[2][5, :3] = -(1 << 23)

    def rows_just_fit(ax, ay):
        ax[2][5, :] = 0
        ax[2][5, 0], ax[2][5, 1] = (1 << 23) - 1, ((1 << 31) - (1 << 21) - 1) // 255 - ((1 << 23) - 1)
        ay[2][5, :] = 0
        ay[2][5, 0], ay[2][5, 1] = -(1 << 23), -(((1 << 31) - 1) // 255 - (1 << 23))

    for pix in (_lib.PIX_U8, _lib.PIX_F16):
        for kw, word in ((dict(pix_fmt=7), "pixel format"), (dict(dst=(0, 8)), "sizes"), (dict(dst=(8, 32768)), "sizes"), (dict(dst=(32768, 8)), "sizes"),
                         (dict(null=True), "null"), (dict(mutate=moves_back), "y tables"), (dict(mutate=count_over_ksize), "x tables"),
                         (dict(mutate=k_too_large), "2^23"), (dict(mutate=k_too_small), "2^23"),
                         (dict(mutate=positive_row_leaves_int32), "int32"), (dict(mutate=negative_row_leaves_int32), "int32")):
            args = dict(src=(12, 20), dst=(30, 31), pix_fmt=pix)
            args.update(kw)
            rc, plan, msg = _create(lib, **args)
            assert rc == _lib.E_INVALID and not plan.value and word in msg, (kw, rc, plan.value, msg)
    rc, plan, msg = _create(lib, (12, 20), (30, 31), no_out=True)
    assert rc == _lib.E_INVALID and "out_plan" in msg
    # the largest rows that are admitted pass the table checks: what is left to fail without a device is the device itself
    import torch
    if not torch.cuda.is_available():
        for pix in (_lib.PIX_U8, _lib.PIX_F16):
            rc, plan, msg = _create(lib, (12, 20), (30, 31), pix_fmt=pix, mutate=rows_just_fit)
            assert rc == _lib.E_HIP and not plan.value and "int32" not in msg, (rc, msg)
    assert lib.crtfx_resample_destroy(None) == _lib.OK and lib.crtfx_resample_set_option(None, 1, 1) == _lib.E_INVALID
    assert lib.crtfx_resample_run(None, None, 0, None, 0, 1, None) == _lib.E_INVALID
    assert lib.crtfx_resample_last_plan(None, ctypes.create_string_buffer(8), 8) == _lib.E_INVALID


def test_create_without_a_gpu_fails_cleanly():
    import torch
    lib = _lib.load()
    if torch.cuda.is_available():
        rc, plan, msg = _create(lib, (12, 20), (30, 31), device=4096)              # no such device on any box
        assert rc == _lib.E_HIP and not plan.value and "4096" in msg
        return
    for filter in model.FILTERS:
        rc, plan, msg = _create(lib, (12, 20), (30, 31), filter=filter)
        assert rc == _lib.E_HIP and not plan.value and msg, (rc, msg)


def test_the_bilinear_stages_still_refuse_a_negative_coefficient():
    """crtfx_ingest_create and crtfx_resize16_create are untouched: a signed table — a real bicubic one, or a bilinear one with one
    coefficient negated — is INVALID there, before a device is touched."""
    lib = _lib.load()

    def negate_one(ax, ay):
        ax[2][5, 0] = -1

    def bicubic(ax, ay):
        for a, n_in, n_out in ((ax, 20, 31), (ay, 12, 30)):
            b = tables.pil_filter_axis(n_in, n_out, "bicubic")
            assert b[2].min() < 0
            a[0][:], a[1][:] = b[0], np.minimum(b[1], a[2].shape[1])
            a[2][:] = b[2][:, :a[2].shape[1]]
    for family, pix in (("ingest", _lib.PIX_U8), ("resize16", _lib.PIX_F16)):
        for mutate in (negate_one, bicubic):
            rc, plan, msg = _create(lib, (12, 20), (30, 31), pix_fmt=pix, mutate=mutate, family=family)
            assert rc == _lib.E_INVALID and not plan.value and "coefficient" in msg, (family, rc, msg)


def _no_device(monkeypatch):
    import torch

    def no_device(*a, **k):
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(_lib, "load", no_device)


def test_the_class_refuses_bad_arguments_before_a_device_is_touched(monkeypatch):
    import torch
    import pythoncrt_amd as pc
    _no_device(monkeypatch)
    for bad in ("nearest", "Lanczos", None):
        with pytest.raises(ValueError, match="filter"):
            pc.Resample("cuda:0", (12, 20), (30, 31), filter=bad)
    for bad in (torch.float32, torch.int8, torch.bfloat16):
        with pytest.raises(ValueError, match="dtype"):
            pc.Resample("cuda:0", (12, 20), (30, 31), dtype=bad)


def test_process_frames_refuses_bad_filters_before_a_device_is_touched(monkeypatch):
    """An unknown name of either filter, and a deliver_filter other than "bilinear" without a deliver_size that differs from the render
    size, are ValueError, raised before a frame is read and before the device is asked for."""
    import pythoncrt_amd as pc

    def never():
        raise AssertionError("a frame was read")
        yield
    _no_device(monkeypatch)
    for fmts in ({}, dict(in_pix_fmt="p010le", out_pix_fmt="p010le"), dict(in_pix_fmt="yuv420p", out_pix_fmt="nv12")):
        for kw, word in ((dict(in_filter="nearest"), "in_filter"), (dict(deliver_filter="cubic", deliver_size=(23, 40)), "deliver_filter"),
                         (dict(in_filter=None), "in_filter"), (dict(deliver_filter="lanczos"), "deliver_filter"),
                         (dict(deliver_filter="bicubic", deliver_size=(46, 80)), "deliver_filter"), (dict(deliver_filter="box", deliver_size=None), "deliver_filter")):
            with pytest.raises(ValueError, match=word):
                pc.process_frames(never(), lambda a: None, 80, 46, 30.0, 1, **kw, **fmts)
    with pytest.raises(ValueError, match="in_size"):                                  # in_size for a 10-bit input stays refused, whatever the filter
        pc.process_frames(never(), lambda a: None, 80, 46, 30.0, 1, in_pix_fmt="p010le", out_pix_fmt="p010le", in_size=(23, 40), in_filter="lanczos")


def test_cli_filter_flags(tmp_path, monkeypatch):
    """--in-filter / --deliver-filter take the five names (default bilinear) and nothing else; --deliver-filter needs a delivery size other
    than the render size; the sharded CLI refuses a non-default value of either.  No output file is created by a refused command."""
    from pythoncrt_amd import cli
    src = tmp_path / "in.rgb"
    src.write_bytes(bytes(46 * 80 * 3))
    base = ["--input", str(src), "--output", str(tmp_path / "out.rgb"), "--width", "80", "--height", "46"]
    parser = cli.add_input_flags(cli.add_output_flags(cli.build_parser()))
    a = parser.parse_args(base)
    assert (a.in_filter, a.deliver_filter) == ("bilinear", "bilinear")
    for flag in ("--in-filter", "--deliver-filter"):
        action = next(x for x in parser._actions if flag in x.option_strings)
        assert tuple(action.choices) == tables.RESAMPLE_FILTERS and action.default == "bilinear"
        with pytest.raises(SystemExit) as e:
            cli.main(base + [flag, "nearest"])
        assert e.value.code not in (0, None)
    for extra in (["--deliver-filter", "lanczos"], ["--deliver-filter", "bicubic", "--deliver-width", "80", "--deliver-height", "46"]):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code not in (0, None) and "--deliver-filter" in str(e.value), extra
    monkeypatch.setenv("CRTFX_FORCE_DIST", "1")
    for extra in (["--in-filter", "bicubic"], ["--deliver-filter", "bilinear", "--in-filter", "box"],
                  ["--deliver-filter", "lanczos"]):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code not in (0, None) and "sharded CLI" in str(e.value) and extra[-2] in str(e.value), extra
    assert not (tmp_path / "out.rgb").exists()


# what include/crtfx_resample.h states for the nine builds: VGPRs as built, (u8, half, half under ACC64)
HEADER_VGPRS = {"k_resample_fused": (43, 56, 43), "k_resample_h": (29, 40, 18), "k_resample_v": (6, 8, 7)}
BUILDS = ("<unsigned char, crtfx_resample_impl::AccU8>", "<unsigned short, crtfx_resample_impl::AccAB>", "<unsigned short, crtfx_resample_impl::Acc64>")


def test_resample_kernels_hold_the_register_budget_and_the_header():
    """Registers and scratch of the nine builds — three kernels x (uint8, half with two int32 accumulators, half with an int64 one) — read
    from the built library's code objects (tools/kernel_resources.py): at most 64 VGPRs (eight waves per SIMD), no AGPRs, no spills, no
    scratch memory, no static LDS (the fused kernel's block is dynamic: its size is the plan's `lds`) — and the figures the header quotes
    are the figures of this build."""
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n.split("::", 1)[1]: v for n, v in res.items() if n.startswith("crtfx_resample_impl::")}
    assert set(found) == {k + b for k in HEADER_VGPRS for b in BUILDS}, sorted(found)
    hdr = open(os.path.join(ROOT, "include", "crtfx_resample.h")).read()
    for kernel, figures in HEADER_VGPRS.items():
        for build, figure in zip(BUILDS, figures):
            v = found[kernel + build]
            assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (kernel, build, v)
            assert v["group_segment_fixed_size"] == 0 and v["agpr_count"] == 0 and v["vgpr_count"] <= 64, (kernel, build, v)
            assert v["vgpr_count"] == figure, (kernel, build, v["vgpr_count"])
        assert re.search(rf"{kernel}\s+u8 {figures[0]}\s+half {figures[1]}\s+half/acc64 {figures[2]}\b", hdr), kernel
    assert "40 960" in hdr and "(32,128) (32,64) (16,128) (16,64) (8,64) (8,32) (4,32)" in hdr


def test_no_packed_shift_clamp_in_the_resample_kernels():
    """The disassembly of the unit's code object holds no v_ashr_pk_* instruction.  The compiler forms one from two neighbouring uint8 clamps
    that are ORed into a dword and then uses its 16-bit result as a whole register; on the MI355X the register's upper half kept what it
    held before, and a byte of every output dword was wrong (see the comment in k_resample_fused's vertical pass)."""
    import subprocess
    import tempfile
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    units = [elf for elf in kernel_resources.code_objects(_lib.LIB_PATH) if b"k_resample_fused" in elf]
    assert len(units) == 1
    with tempfile.NamedTemporaryFile(suffix=".elf") as f:
        f.write(units[0])
        f.flush()
        asm = subprocess.run([kernel_resources._tool("llvm-objdump"), "-d", "--mcpu=gfx950", f.name], capture_output=True, text=True, check=True).stdout
    assert asm.count("v_med3_i32") >= 6 and "v_mad_i32_i24" in asm           # the disassembly is the kernels'
    assert "v_ashr_pk" not in asm
