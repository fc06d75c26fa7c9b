"""The ingest stage without a GPU: the host tables of Pillow's 8-bit BILINEAR resampler (tables.pil_resample_axis) drive an integer numpy
model (tests/pil_resize_model.py) that equals the installed Pillow byte for byte; the C-ABI of include/crtfx_ingest.h is bound symbol for
symbol and fails cleanly without a device; the new kernels use no scratch memory."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pythoncrt_amd import _lib, tables  # noqa: E402
from tests import pil_resize_model as model  # noqa: E402

AXES = sorted({(s[i], d[i]) for s, d in model.PAIRS + model.EXTRA_PAIRS for i in (0, 1)} | {(1080, 2160), (1920, 3840), (2160, 1080), (720, 1080)})


@pytest.mark.parametrize("src,dst", model.PAIRS + model.EXTRA_PAIRS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_model_equals_pillow(src, dst):
    """Image.resize((w, h), Image.BILINEAR) of the Pillow installed here == the two integer passes over pil_resample_axis's tables: 0 bytes
    differ, for every pair and both images."""
    for name, img in model.images(*src).items():
        got, exp = model.resize(img, *dst), model.pillow(img, *dst)
        assert got.shape == exp.shape == (dst[0], dst[1], 3) and got.dtype == np.uint8
        assert int((got != exp).sum()) == 0, (src, dst, name, int((got != exp).sum()))


def test_there_are_the_twelve_pairs_and_the_gpu_extras():
    assert len(model.PAIRS) == 12 and ((360, 640), (9, 16)) in model.EXTRA_PAIRS
    assert {(s[1], d[1]) for s, d in model.EXTRA_PAIRS[1:]} == {(61, 85), (62, 86), (63, 87), (64, 88)}


@pytest.mark.parametrize("n_in,n_out", AXES, ids=lambda n: str(n))
def test_axis_tables_keep_the_rules_the_kernels_rest_on(n_in, n_out):
    """Shapes and dtypes; every tap window inside the source; windows move forward only (a tile's source extent is first tap .. last tap);
    coefficients non-negative and below 2^24 (24-bit multiplies); a row sums to 2^22 within +-ksize (each tap rounds once); the int32
    accumulator of a pass cannot wrap."""
    xmin, count, k = tables.pil_resample_axis(n_in, n_out)
    scale = max(n_in / n_out, 1.0)
    ksize = int(np.ceil(scale)) * 2 + 1
    assert xmin.dtype == count.dtype == k.dtype == np.int32 and xmin.shape == count.shape == (n_out,) and k.shape == (n_out, ksize)
    assert all(a.flags["C_CONTIGUOUS"] for a in (xmin, count, k))
    assert xmin.min() >= 0 and count.min() >= 1 and count.max() <= ksize and (xmin + count).max() <= n_in
    assert (np.diff(xmin) >= 0).all() and (np.diff(xmin + count) >= 0).all()
    assert k.min() >= 0 and k.max() < 1 << 24
    assert (k[np.arange(ksize)[None, :] >= count[:, None]] == 0).all()
    sums = k.astype(np.int64).sum(axis=1)
    assert np.abs(sums - (1 << 22)).max() <= ksize, int(np.abs(sums - (1 << 22)).max())
    assert (1 << 21) + 255 * int(sums.max()) < 2 ** 31


@pytest.mark.parametrize("n", [1, 2, 40, 1080])
def test_an_unchanged_axis_is_the_identity(n):
    xmin, count, k = tables.pil_resample_axis(n, n)
    assert k.shape == (n, 3) and (k == np.array([1 << 22, 0, 0], np.int32)).all()
    assert np.array_equal(xmin, np.arange(n, dtype=np.int32))
    img = model.images(n, 5)["random"]
    assert np.array_equal(model.resample_pass(np.ascontiguousarray(img.transpose(1, 0, 2)), xmin, count, k).transpose(1, 0, 2), img)


def test_bad_axis_sizes_raise():
    for bad in ((0, 4), (4, 0), (-1, 3)):
        with pytest.raises(ValueError):
            tables.pil_resample_axis(*bad)


def test_header_prototypes_are_the_bound_symbols():
    """include/crtfx_ingest.h declares exactly _lib.INGEST_SYMBOLS (argument counts included), apart from crtfx.h's own table, and the built
    library exports every one."""
    hdr = open(os.path.join(ROOT, "include", "crtfx_ingest.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_ingest_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(_lib.INGEST_SYMBOLS), set(protos) ^ set(_lib.INGEST_SYMBOLS)
    assert not set(_lib.INGEST_SYMBOLS) & set(_lib.SYMBOLS)
    for name, args in protos.items():
        n_args = 0 if args.strip() in ("", "void") else len(args.split(","))
        assert n_args == len(_lib.INGEST_SYMBOLS[name][1]), name
    assert all(os.path.basename(f) in {os.path.basename(s) for s in _lib.SOURCES} for f in ("crtfx_ingest.hip", "crtfx_ingest.h"))
    lib = _lib.load()
    for name in _lib.INGEST_SYMBOLS:
        assert getattr(lib, name).argtypes == _lib.INGEST_SYMBOLS[name][1]


def _create(lib, src, dst, pix_fmt=_lib.PIX_U8, device=0, mutate=None, null=False):
    ax, ay = tables.pil_resample_axis(src[1], max(1, dst[1])), tables.pil_resample_axis(src[0], max(1, dst[0]))
    if mutate:
        mutate(ax, ay)
    plan = ctypes.c_void_p(1)
    rc = lib.crtfx_ingest_create(device, src[0], src[1], dst[0], dst[1], pix_fmt, None if null else tables.ptr(ax[0]), tables.ptr(ax[1]), tables.ptr(ax[2]),
                                 ax[2].shape[1], tables.ptr(ay[0]), tables.ptr(ay[1]), tables.ptr(ay[2]), ay[2].shape[1], ctypes.byref(plan))
    return rc, plan, (lib.crtfx_ingest_last_error(None) or b"").decode()


def test_create_refuses_bad_arguments_before_it_touches_a_device():
    """The argument checks of crtfx_ingest_create come first, so they hold on any machine: half frames are UNSUPPORTED, sizes < 1, a null
    table and a table whose tap window leaves the source are INVALID; each leaves *out_plan NULL and a message."""
    lib = _lib.load()

    def window_leaves(ax, ay):
        ax[0][-1] += 5

    def moves_back(ax, ay):
        ay[0][1] = ay[0][2] + 1

    for kw, code, word in ((dict(pix_fmt=_lib.PIX_F16), _lib.E_UNSUPPORTED, "uint8"), (dict(dst=(0, 8)), _lib.E_INVALID, "sizes"),
                           (dict(dst=(8, 40000)), _lib.E_INVALID, "sizes"), (dict(null=True), _lib.E_INVALID, "null"),
                           (dict(pix_fmt=7), _lib.E_INVALID, "pixel format"), (dict(mutate=window_leaves), _lib.E_INVALID, "x tables"),
                           (dict(mutate=moves_back), _lib.E_INVALID, "y tables")):
        args = dict(src=(12, 20), dst=(30, 31))
        args.update(kw)
        rc, plan, msg = _create(lib, **args)
        assert rc == code and not plan.value and word in msg, (kw, rc, plan.value, msg)
    assert lib.crtfx_ingest_destroy(None) == _lib.OK and lib.crtfx_ingest_set_option(None, 1, 1) == _lib.E_INVALID
    assert lib.crtfx_ingest_run(None, None, 0, None, 0, 1, None) == _lib.E_INVALID


def test_create_without_a_gpu_fails_cleanly():
    import torch
    if torch.cuda.is_available():
        lib = _lib.load()
        rc, plan, msg = _create(lib, (12, 20), (30, 31), device=4096)              # no such device on any box
        assert rc == _lib.E_HIP and not plan.value and "4096" in msg
        return
    lib = _lib.load()
    rc, plan, msg = _create(lib, (12, 20), (30, 31))
    assert rc == _lib.E_HIP and not plan.value and msg, (rc, msg)


def test_ingest_kernels_have_no_scratch_and_no_spills():
    """Registers and scratch of the three new kernels, read from the built library's code objects (tools/kernel_resources.py): no spills, no
    scratch memory, no static LDS (the fused kernel's block is dynamic: its size is the plan's `lds`), and few enough VGPRs (<= 64) for
    eight waves per SIMD."""
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n: v for n, v in res.items() if n.startswith("crtfx_ingest_impl::")}
    assert set(found) == {"crtfx_ingest_impl::k_ingest_fused", "crtfx_ingest_impl::k_ingest_h", "crtfx_ingest_impl::k_ingest_v"}, sorted(found)
    for name, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == 0 and v["vgpr_count"] + v["agpr_count"] <= 64, (name, v)
