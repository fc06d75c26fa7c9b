"""The egress stage without a GPU: tables.yuv_matrix against the four literal matrices of tests/yuv_model.py, the identities the arithmetic
rests on, the integer model against its float64 restatement, the layout of a frame, the C-ABI of include/crtfx_egress.h bound symbol for
symbol and failing cleanly without a device, the kernels' registers, and the sharded CLI's refusal."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pythoncrt_amd import _lib, egress, tables  # noqa: E402
from tests import yuv_model as model  # noqa: E402


def _uniform(colours):
    """A 2 x (2 * n) frame whose 2 x 2 blocks are the n colours."""
    c = np.asarray(colours, dtype=np.uint8).reshape(-1, 3)
    return np.repeat(np.repeat(c[None, :, :], 2, axis=1), 2, axis=0)


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_yuv_matrix_equals_the_literals_and_keeps_the_row_sums(matrix, rng):
    m, off = tables.yuv_matrix(matrix, rng)
    assert m.dtype == off.dtype == np.int32 and m.shape == (9,) and off.shape == (3,) and m.flags["C_CONTIGUOUS"]
    assert m.reshape(3, 3).tolist() == [list(r) for r in model.MATRICES[(matrix, rng)]]
    assert tuple(off.tolist()) == model.OFFSETS[rng]
    sy = 219.0 / 255.0 if rng == "tv" else 1.0
    rows = m.reshape(3, 3).astype(np.int64)
    assert rows[0].sum() == int(np.floor(sy * 65536 + 0.5)) and rows[1].sum() == 0 and rows[2].sum() == 0
    # every entry but G is the rounded float64 coefficient; G moved by the adjustment by at most 2
    want = np.floor(model.float_matrix(matrix, rng) * 65536 + 0.5).astype(np.int64)
    assert np.array_equal(rows[:, [0, 2]], want[:, [0, 2]]) and np.abs(rows[:, 1] - want[:, 1]).max() <= 2
    # the accumulators stay inside [0, 2^31): the rule crtfx_egress_create checks
    for row, konst, x in ((rows[0], (int(off[0]) << 16) + (1 << 15), 255), (rows[1], (128 << 18) + (1 << 17), 1020), (rows[2], (128 << 18) + (1 << 17), 1020)):
        assert konst + row[row < 0].sum() * x >= 0 and konst + row[row > 0].sum() * x < 2 ** 31


def test_yuv_matrix_refuses_unknown_names():
    for bad in (("bt2020", "tv"), ("bt601", "full")):
        with pytest.raises(ValueError):
            tables.yuv_matrix(*bad)


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_greys_black_white_and_the_clamp_colours(matrix, rng):
    greys = [(g, g, g) for g in range(256)]
    y, u, v = model.convert(_uniform(greys), matrix, rng)
    assert (u == 128).all() and (v == 128).all()
    assert (int(y[0, 0]), int(y[0, -1])) == ((16, 235) if rng == "tv" else (0, 255))
    assert (np.diff(y[0, ::2].astype(int)) >= 0).all()
    if rng == "pc":
        assert np.array_equal(y[0, ::2], np.arange(256))             # full range: a grey's luma is the grey
        # the upper clamp is live: pure blue's U and pure red's V are 256 before it
        m = np.array(model.MATRICES[(matrix, rng)], dtype=np.int64)
        for colour, row in (((0, 0, 255), 1), ((255, 0, 0), 2)):
            s = 4 * np.array(colour, dtype=np.int64)
            assert (s @ m[row] + (128 << 18) + (1 << 17)) >> 18 == 256
        _, u, v = model.convert(_uniform([(0, 0, 255), (255, 0, 0)]), matrix, rng)
        assert int(u[0, 0]) == 255 and int(v[0, 1]) == 255


def _lattice():
    steps = np.rint(np.linspace(0, 255, 33)).astype(np.uint8)
    assert len(set(steps.tolist())) == 33
    lat = np.stack(np.meshgrid(steps, steps, steps, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.concatenate([lat, np.array([(g, g, g) for g in range(256)], dtype=np.uint8), np.array(model.CLAMP_COLOURS, dtype=np.uint8)])


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_integer_model_against_the_float_restatement(matrix, rng):
    """A 33-step lattice, every grey and the cube corners: the integer result is the float64 one (round-half-up of F . rgb + off, clamped)
    except where the float value sits within 3 * 255 * 2^-16 of a half-integer — the most the rounding of three coefficients to 2^-16 plus
    the G adjustment can move a sum of three samples — and there it differs by one code."""
    img = _uniform(_lattice())
    got = model.convert(img, matrix, rng)
    exp, raw = model.convert_float(img, matrix, rng)
    bound = 3 * 255 * 2.0 ** -16
    for g, e, r in zip(got, exp, raw):
        d = g.astype(np.int64) - e.astype(np.int64)
        assert np.abs(d).max() <= 1
        dist = np.abs(r - np.floor(r) - 0.5)
        assert (dist[d != 0] <= bound).all(), float(dist[d != 0].max())


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_a_uniform_block_has_the_per_pixel_chroma(matrix, rng):
    cols = _lattice()[::7]
    _, u, v = model.convert(_uniform(cols), matrix, rng)
    m, off = np.array(model.MATRICES[(matrix, rng)], dtype=np.int64), model.OFFSETS[rng]
    c = cols.astype(np.int64)
    for plane, row in ((u, 1), (v, 2)):
        per_pixel = np.clip((c @ m[row] + (off[row] << 16) + (1 << 15)) >> 16, 0, 255)
        assert np.array_equal(plane[0], per_pixel)


@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (3, 5), (37, 131), (16, 64), (1080, 1920)])
def test_frame_bytes_and_plane_offsets(h, w):
    ch, cw, fb = model.sizes(h, w)
    assert egress.frame_bytes(h, w) == fb == h * w + 2 * ch * cw and (ch, cw) == (-(-h // 2), -(-w // 2))
    if h * w > 10000:
        return
    img = model.images(h, w)[0]
    y, u, v = model.convert(img)
    p = model.pack(img, "yuv420p")
    assert p.shape == (fb,) and p.dtype == np.uint8
    py, pu, pv = egress.split_planes(p, (h, w), "yuv420p")
    assert np.array_equal(py, y) and np.array_equal(pu, u) and np.array_equal(pv, v)
    assert np.array_equal(p[h * w:h * w + ch * cw].reshape(ch, cw), u) and np.array_equal(p[h * w + ch * cw:].reshape(ch, cw), v)
    q = model.pack(img, "nv12")
    qy, quv = egress.split_planes(q, (h, w), "nv12")
    assert np.array_equal(qy, y) and np.array_equal(quv[..., 0], u) and np.array_equal(quv[..., 1], v)
    assert np.array_equal(q[h * w::2].reshape(ch, cw), u) and np.array_equal(q[h * w + 1::2].reshape(ch, cw), v)
    # odd edges replicate the last row / column
    if h % 2 and w % 2:
        s = model.box_sum(img)
        assert np.array_equal(s[-1, -1], 4 * img[-1, -1].astype(np.int64))
    with pytest.raises(ValueError):
        egress.split_planes(p[:-1], (h, w), "yuv420p")


def test_header_prototypes_are_the_bound_symbols():
    """include/crtfx_egress.h declares exactly _lib.EGRESS_SYMBOLS (argument counts included); both new files are kernel sources of the build;
    the built library exports every symbol."""
    hdr = open(os.path.join(ROOT, "include", "crtfx_egress.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_egress_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(_lib.EGRESS_SYMBOLS), set(protos) ^ set(_lib.EGRESS_SYMBOLS)
    assert not set(_lib.EGRESS_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.INGEST_SYMBOLS))
    for name, args in protos.items():
        n_args = 0 if args.strip() in ("", "void") else len(args.split(","))
        assert n_args == len(_lib.EGRESS_SYMBOLS[name][1]), name
    assert all(os.path.basename(f) in {os.path.basename(s) for s in _lib.SOURCES} for f in ("crtfx_egress.hip", "crtfx_egress.h"))
    lib = _lib.load()
    for name in _lib.EGRESS_SYMBOLS:
        assert getattr(lib, name).argtypes == _lib.EGRESS_SYMBOLS[name][1]


def _create(lib, h=12, w=20, pix_fmt=_lib.PIX_U8, layout=_lib.EGRESS_NV12, device=0, m=None, off=None, null=False):
    tm, toff = tables.yuv_matrix("bt601", "tv")
    m = tm if m is None else np.ascontiguousarray(m, dtype=np.int32)
    off = toff if off is None else np.ascontiguousarray(off, dtype=np.int32)
    plan = ctypes.c_void_p(1)
    rc = lib.crtfx_egress_create(device, h, w, pix_fmt, layout, None if null else tables.ptr(m), tables.ptr(off), ctypes.byref(plan))
    return rc, plan, (lib.crtfx_egress_last_error(None) or b"").decode()


def test_create_refuses_bad_arguments_before_it_touches_a_device():
    """The argument checks of crtfx_egress_create come first, so they hold on any machine: half frames are UNSUPPORTED; a size < 1 or
    > 32767, an unknown layout, a null table, an offset outside 0..255 and a matrix whose accumulator could leave [0, 2^31) are INVALID;
    each leaves *out_plan NULL and a message."""
    lib = _lib.load()
    good = tables.yuv_matrix("bt601", "pc")[0]
    too_big, goes_negative = good.copy(), good.copy()
    too_big[0] = 1 << 23                                      # 255 * 2^23 alone is 2^31 - 2^23; with G and B the Y accumulator passes 2^31
    goes_negative[4] -= 12000                                 # U row: 128 << 18 no longer covers 1020 * (sum of the negative entries)
    for kw, code, word in ((dict(pix_fmt=_lib.PIX_F16), _lib.E_UNSUPPORTED, "uint8"), (dict(h=0), _lib.E_INVALID, "size"),
                           (dict(w=40000), _lib.E_INVALID, "size"), (dict(null=True), _lib.E_INVALID, "null"),
                           (dict(pix_fmt=7), _lib.E_INVALID, "pixel format"), (dict(layout=2), _lib.E_INVALID, "layout"),
                           (dict(off=(16, 256, 128)), _lib.E_INVALID, "offset"), (dict(m=too_big), _lib.E_INVALID, "accumulator"),
                           (dict(m=goes_negative), _lib.E_INVALID, "accumulator")):
        rc, plan, msg = _create(lib, **kw)
        assert rc == code and not plan.value and word in msg, (kw, rc, plan.value, msg)
    assert lib.crtfx_egress_destroy(None) == _lib.OK and lib.crtfx_egress_set_option(None, 1, 1) == _lib.E_INVALID
    assert lib.crtfx_egress_run(None, None, 0, None, 0, 1, None) == _lib.E_INVALID and lib.crtfx_egress_frame_bytes(None) == 0


def test_create_without_a_gpu_fails_cleanly():
    import torch
    lib = _lib.load()
    if torch.cuda.is_available():
        rc, plan, msg = _create(lib, device=4096)               # no such device on any box
        assert rc == _lib.E_HIP and not plan.value and "4096" in msg
        return
    rc, plan, msg = _create(lib)
    assert rc == _lib.E_HIP and not plan.value and msg, (rc, msg)


def test_egress_kernels_have_no_scratch_and_no_spills():
    """Registers and scratch of the four kernel builds (two paths x two layouts), read from the built library's code objects
    (tools/kernel_resources.py): no spills, no scratch memory, no LDS, and at most 64 VGPRs (eight waves per SIMD)."""
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n: v for n, v in res.items() if n.startswith("crtfx_egress_impl::")}
    assert set(found) == {f"crtfx_egress_impl::k_egress_420_{p}<{l}>" for p in ("vec", "general") for l in ("true", "false")}, sorted(found)
    for name, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == 0 and v["vgpr_count"] + v["agpr_count"] <= 64, (name, v)


def test_sharded_cli_refuses_a_yuv_output_before_it_touches_a_device(monkeypatch, tmp_path):
    """One process per GPU writes rgb24 at per-rank offsets: with --out-pix-fmt nv12 the sharded CLI exits with a message that names the
    flag — before torch.distributed or a device is touched (it does so on a machine without a GPU, and without a launcher)."""
    from pythoncrt_amd import cli
    src = tmp_path / "in.rgb"
    src.write_bytes(bytes(8 * 8 * 3))
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:
        cli.main(["--input", str(src), "--output", str(tmp_path / "out.yuv"), "--width", "8", "--height", "8", "--out-pix-fmt", "nv12"])
    assert "--out-pix-fmt nv12" in str(e.value) and "sharded" in str(e.value)
    assert not (tmp_path / "out.yuv").exists()
    a = cli.add_output_flags(cli.build_parser()).parse_args(["--input", "x"])
    assert (a.out_pix_fmt, a.out_matrix, a.out_range) == ("rgb24", "bt601", "tv")
    with pytest.raises(SystemExit):
        cli.add_output_flags(cli.build_parser()).parse_args(["--input", "x", "--out-pix-fmt", "yuv444p"])
