"""The source stage without a GPU: tables.rgb_matrix against the four literal matrices of tests/unpack_model.py, the identities the
arithmetic rests on, the integer model against its float64 restatement, the round trip through the egress model, the layout of a frame, the
C-ABI of include/crtfx_unpack.h bound symbol for symbol and failing cleanly without a device, the kernels' registers, the sharded CLI's
refusal and iter_yuv420."""
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
from tests import unpack_model as model  # noqa: E402
from tests import yuv_model  # noqa: E402


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_rgb_matrix_equals_the_literals(matrix, rng):
    m, off = tables.rgb_matrix(matrix, rng)
    assert m.dtype == off.dtype == np.int32 and m.shape == (9,) and off.shape == (3,) and m.flags["C_CONTIGUOUS"] and off.flags["C_CONTIGUOUS"]
    rows = m.reshape(3, 3).astype(np.int64)
    assert rows.tolist() == [list(r) for r in model.MATRICES[(matrix, rng)]]
    assert tuple(off.tolist()) == model.OFFSETS[rng]
    assert rows[0, 1] == 0 and rows[2, 2] == 0                                # R/U and B/V: exactly 0
    assert rows[0, 0] == rows[1, 0] == rows[2, 0]                             # one Y entry: every grey gives R = G = B
    # every entry is the rounded float64 coefficient, none adjusted
    assert np.array_equal(rows, np.floor(model.float_matrix(matrix, rng) * 65536 + 0.5).astype(np.int64))
    # the accumulators stay inside int32 (the rule crtfx_unpack_create checks), and within the stated +-3.6e7
    assert (np.abs(rows).sum(axis=1) * 255 + (1 << 15) < 2 ** 31).all()
    lo, hi = -model.OFFSETS[rng][0], 255 - model.OFFSETS[rng][0]
    worst = max(abs(r[0]) * max(-lo, hi) + (abs(r[1]) + abs(r[2])) * 128 + (1 << 15) for r in rows)
    assert worst <= 3.6e7, worst


def test_rgb_matrix_refuses_unknown_names():
    for bad in (("bt2020", "tv"), ("bt601", "full")):
        with pytest.raises(ValueError):
            tables.rgb_matrix(*bad)


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_greys_black_white_and_the_clamp_colours(matrix, rng):
    g = np.arange(256, dtype=np.int64)
    off = model.OFFSETS[rng]
    zero = np.zeros_like(g)
    rgb = model.convert_yuv(g - off[0], zero, zero, matrix, rng)              # U = V = 128
    assert np.array_equal(rgb[:, 0], rgb[:, 1]) and np.array_equal(rgb[:, 1], rgb[:, 2])
    assert (np.diff(rgb[:, 0].astype(int)) >= 0).all()
    if rng == "tv":
        assert rgb[16].tolist() == [0, 0, 0] and rgb[235].tolist() == [255, 255, 255]
        assert rgb[:16].max() == 0 and rgb[235:].min() == 255
    else:
        assert np.array_equal(rgb[:, 0], np.arange(256))                      # full range: a grey's RGB is its Y
    # both clamps are live on the stated colours, before clamping: limited-range white with V = 240 passes 255 in R; Y = 16, U = V = 16 is
    # negative — in R and B (c = 0, d = e = -112, and the R/V and B/U entries are positive; both G entries are negative, so G is positive
    # there, and it is the mirror colour U = V = 240 that is negative in G).  All three colours are in the palette of model.images.
    m = np.array(model.MATRICES[(matrix, "tv")], dtype=np.int64)

    def before_clamp(y, u, v):
        return (m @ np.array([y - 16, u - 128, v - 128], dtype=np.int64) + (1 << 15)) >> 16
    assert before_clamp(235, 128, 240)[0] > 255
    dark = before_clamp(16, 16, 16)
    assert dark[0] < 0 and dark[2] < 0 and dark[1] > 0
    assert before_clamp(16, 240, 240)[1] < 0
    for colour in ((235, 128, 240), (16, 16, 16), (16, 240, 240)):
        assert colour in model.CLAMP_COLOURS
        got = model.convert_yuv(*(np.array([x - o]) for x, o in zip(colour, model.OFFSETS["tv"])), matrix, "tv")[0]
        assert np.array_equal(got, np.clip(before_clamp(*colour), 0, 255))


def _lattice(steps=33):
    s = np.rint(np.linspace(0, 255, steps)).astype(np.int64)
    assert len(set(s.tolist())) == steps
    lat = np.stack(np.meshgrid(s, s, s, indexing="ij"), axis=-1).reshape(-1, 3)
    greys = np.stack([np.arange(256), np.full(256, 128), np.full(256, 128)], axis=1)
    return np.concatenate([lat, greys, np.array(model.CLAMP_COLOURS, dtype=np.int64)])


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_integer_model_against_the_float_restatement(matrix, rng):
    """A 33-step (Y, U, V) lattice, every grey and the clamp colours: the integer result is the float64 one (round-half-up of F . (c, d, e),
    clamped) except where the float value sits within (255 + 128 + 128) * 2^-17 of a half-integer — the most the rounding of three
    coefficients to 2^-16 can move the sum — and there it differs by one code.  (Over all 2^24 triples of all four matrices the largest
    such distance is 0.0016 and the largest difference 1.)"""
    yuv = _lattice()
    off = model.OFFSETS[rng]
    c, d, e = yuv[:, 0] - off[0], yuv[:, 1] - off[1], yuv[:, 2] - off[2]
    got = model.convert_yuv(c, d, e, matrix, rng)
    exp, raw = model.convert_yuv_float(c.astype(np.float64), d.astype(np.float64), e.astype(np.float64), matrix, rng)
    diff = got.astype(np.int64) - exp.astype(np.int64)
    assert np.abs(diff).max() <= 1
    bound = (255 + 128 + 128) * 2.0 ** -17
    dist = np.abs(raw - np.floor(raw) - 0.5)
    assert (dist[diff != 0] <= bound).all(), float(dist[diff != 0].max())


@pytest.mark.parametrize("matrix,rng", model.CASES)
def test_round_trip_through_the_egress_model(matrix, rng):
    """2 x 2 blocks of one colour over a 52-step RGB lattice: unpack(pack(rgb)) is within 2 codes of rgb at limited range and 1 at full
    range — the exact maxima of the two stated arithmetics."""
    s = np.rint(np.linspace(0, 255, 52)).astype(np.uint8)
    cols = np.stack(np.meshgrid(s, s, s, indexing="ij"), axis=-1).reshape(-1, 3)
    img = np.repeat(np.repeat(cols[None, :, :], 2, axis=1), 2, axis=0)        # 2 x (2 n) x 3
    h, w = img.shape[:2]
    for layout in ("yuv420p", "nv12"):
        back = model.unpack(yuv_model.pack(img, layout, matrix, rng), h, w, layout, matrix, rng)
        err = np.abs(back.astype(np.int64) - img.astype(np.int64)).max()
        assert err <= (2 if rng == "tv" else 1), (layout, int(err))


@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (3, 5), (37, 131), (16, 64)])
def test_frame_bytes_plane_offsets_and_replication(h, w):
    from pythoncrt_amd import unpack
    ch, cw, fb = model.sizes(h, w)
    assert unpack.frame_bytes(h, w) == fb == h * w + 2 * ch * cw and (ch, cw) == (-(-h // 2), -(-w // 2))
    p = model.images(h, w)[0]
    assert p.shape == (fb,) and p.dtype == np.uint8
    y, u, v = model.planes(p, h, w, "yuv420p")
    assert np.array_equal(y, p[:h * w].reshape(h, w))
    assert np.array_equal(u, p[h * w:h * w + ch * cw].reshape(ch, cw)) and np.array_equal(v, p[h * w + ch * cw:].reshape(ch, cw))
    q = model.relayout(p, h, w, "nv12")
    assert q.shape == (fb,) and np.array_equal(q[:h * w], p[:h * w])
    assert np.array_equal(q[h * w::2].reshape(ch, cw), u) and np.array_equal(q[h * w + 1::2].reshape(ch, cw), v)
    py, pu, pv = unpack.split_planes(p, (h, w), "yuv420p")
    qy, quv = unpack.split_planes(q, (h, w), "nv12")
    assert np.array_equal(py, y) and np.array_equal(pu, u) and np.array_equal(pv, v)
    assert np.array_equal(qy, y) and np.array_equal(quv[..., 0], u) and np.array_equal(quv[..., 1], v)
    # the same samples give the same RGB in both layouts; the last column / row read the last chroma sample, every pixel reads (y >> 1, x >> 1)
    a, b = model.unpack(p, h, w, "yuv420p"), model.unpack(q, h, w, "nv12")
    assert a.shape == (h, w, 3) and a.dtype == np.uint8 and np.array_equal(a, b)
    c, d, e = model.terms(p, h, w, "yuv420p", "tv")
    assert d[h - 1, w - 1] == int(u[ch - 1, cw - 1]) - 128 and e[h - 1, w - 1] == int(v[ch - 1, cw - 1]) - 128
    for yy, xx in ((0, 0), (h - 1, 0), (0, w - 1), (h // 2, w // 2)):
        assert d[yy, xx] == int(u[yy >> 1, xx >> 1]) - 128 and e[yy, xx] == int(v[yy >> 1, xx >> 1]) - 128 and c[yy, xx] == int(y[yy, xx]) - 16


def test_header_prototypes_are_the_bound_symbols():
    """include/crtfx_unpack.h declares exactly _lib.UNPACK_SYMBOLS (argument counts included), argument for argument the seven of
    crtfx_egress.h; the table is disjoint from the other three; both new files are kernel sources of the build; the built library exports
    every symbol."""
    hdr = open(os.path.join(ROOT, "include", "crtfx_unpack.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_unpack_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(_lib.UNPACK_SYMBOLS), set(protos) ^ set(_lib.UNPACK_SYMBOLS)
    assert not set(_lib.UNPACK_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.INGEST_SYMBOLS) | set(_lib.EGRESS_SYMBOLS))
    for name, args in protos.items():
        n_args = 0 if args.strip() in ("", "void") else len(args.split(","))
        assert n_args == len(_lib.UNPACK_SYMBOLS[name][1]), name
        twin = name.replace("crtfx_unpack_", "crtfx_egress_")
        assert _lib.UNPACK_SYMBOLS[name] == _lib.EGRESS_SYMBOLS[twin], name
    for other in ("crtfx.h", "crtfx_ingest.h", "crtfx_egress.h"):
        assert "crtfx_unpack" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert (_lib.UNPACK_YUV420P, _lib.UNPACK_NV12, _lib.UNPACK_OPT_FORCE_GENERAL) == (0, 1, 1)
    assert all(os.path.basename(f) in {os.path.basename(s) for s in _lib.SOURCES} for f in ("crtfx_unpack.hip", "crtfx_unpack.h"))
    lib = _lib.load()
    for name in _lib.UNPACK_SYMBOLS:
        assert getattr(lib, name).argtypes == _lib.UNPACK_SYMBOLS[name][1]


def _create(lib, h=12, w=20, pix_fmt=_lib.PIX_U8, layout=_lib.UNPACK_NV12, device=0, m=None, off=None, null=False):
    tm, toff = tables.rgb_matrix("bt601", "tv")
    m = tm if m is None else np.ascontiguousarray(m, dtype=np.int32)
    off = toff if off is None else np.ascontiguousarray(off, dtype=np.int32)
    plan = ctypes.c_void_p(1)
    rc = lib.crtfx_unpack_create(device, h, w, pix_fmt, layout, None if null else tables.ptr(m), tables.ptr(off), ctypes.byref(plan))
    return rc, plan, (lib.crtfx_unpack_last_error(None) or b"").decode()


def test_create_refuses_bad_arguments_before_it_touches_a_device():
    """The argument checks of crtfx_unpack_create come first, so they hold on any machine: half frames are UNSUPPORTED; a size < 1 or
    > 32767, an unknown layout or pixel format, a null table, an offset outside 0..255 and a matrix whose accumulator could leave int32 are
    INVALID; each leaves *out_plan NULL and a message."""
    lib = _lib.load()
    good = tables.rgb_matrix("bt601", "tv")[0]
    too_big, too_negative, just_fits = good.copy(), good.copy(), good.copy()
    too_big[0] = 1 << 23                                      # R row: 255 * (2^23 + 104597) + 2^15 passes 2^31
    too_negative[4] = -(1 << 23)                              # G row: the rule sums magnitudes
    just_fits[0:3] = (8421375, 0, 0)                          # 255 * 8421375 + 2^15 = 2^31 - 255: admitted (no device here: E_HIP, or a plan)
    for kw, code, word in ((dict(pix_fmt=_lib.PIX_F16), _lib.E_UNSUPPORTED, "uint8"), (dict(h=0), _lib.E_INVALID, "size"),
                           (dict(w=40000), _lib.E_INVALID, "size"), (dict(h=32768), _lib.E_INVALID, "size"), (dict(null=True), _lib.E_INVALID, "null"),
                           (dict(pix_fmt=7), _lib.E_INVALID, "pixel format"), (dict(layout=2), _lib.E_INVALID, "layout"),
                           (dict(off=(16, 256, 128)), _lib.E_INVALID, "offset"), (dict(off=(-1, 128, 128)), _lib.E_INVALID, "offset"),
                           (dict(m=too_big), _lib.E_INVALID, "accumulator"), (dict(m=too_negative), _lib.E_INVALID, "accumulator")):
        rc, plan, msg = _create(lib, **kw)
        assert rc == code and not plan.value and word in msg, (kw, rc, plan.value, msg)
    rc, plan, msg = _create(lib, m=just_fits)
    assert rc in (_lib.OK, _lib.E_HIP), (rc, msg)
    if rc == _lib.OK:
        assert lib.crtfx_unpack_destroy(plan) == _lib.OK
    assert lib.crtfx_unpack_destroy(None) == _lib.OK and lib.crtfx_unpack_set_option(None, 1, 1) == _lib.E_INVALID
    assert lib.crtfx_unpack_run(None, None, 0, None, 0, 1, None) == _lib.E_INVALID and lib.crtfx_unpack_frame_bytes(None) == 0
    assert lib.crtfx_unpack_last_plan(None, ctypes.create_string_buffer(8), 8) == _lib.E_INVALID


def test_create_without_a_gpu_fails_cleanly():
    import torch
    lib = _lib.load()
    if torch.cuda.is_available():
        rc, plan, msg = _create(lib, device=4096)               # no such device on any box
        assert rc == _lib.E_HIP and not plan.value and "4096" in msg
        return
    rc, plan, msg = _create(lib)
    assert rc == _lib.E_HIP and not plan.value and msg, (rc, msg)


def test_unpack_kernels_have_no_scratch_and_no_spills():
    """Registers and scratch of the four kernel builds (two paths x two layouts), read from the built library's code objects
    (tools/kernel_resources.py): no spills, no scratch memory, no LDS, and at most 64 VGPRs + AGPRs (eight waves per SIMD)."""
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n: v for n, v in res.items() if n.startswith("crtfx_unpack_impl::")}
    assert set(found) == {f"crtfx_unpack_impl::k_unpack_420_{p}<{l}>" for p in ("vec", "general") for l in ("true", "false")}, sorted(found)
    for name, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == 0 and v["vgpr_count"] + v["agpr_count"] <= 64, (name, v)


def test_sharded_cli_refuses_a_yuv_input_before_it_touches_a_device(monkeypatch, tmp_path):
    """One process per GPU reads rgb24 at per-rank offsets: with --in-pix-fmt nv12 the sharded CLI exits with a message that names the flag
    — before torch.distributed or a device is touched (it does so on a machine without a GPU, and without a launcher)."""
    from pythoncrt_amd import cli
    src = tmp_path / "in.yuv"
    src.write_bytes(bytes(8 * 8 * 3 // 2))
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:
        cli.main(["--input", str(src), "--output", str(tmp_path / "out.rgb"), "--width", "8", "--height", "8", "--in-pix-fmt", "nv12"])
    assert "--in-pix-fmt nv12" in str(e.value) and "sharded" in str(e.value)
    assert not (tmp_path / "out.rgb").exists()
    a = cli.add_input_flags(cli.build_parser()).parse_args(["--input", "x"])
    assert (a.in_pix_fmt, a.in_matrix, a.in_range) == ("rgb24", "bt601", "tv")
    with pytest.raises(SystemExit):
        cli.add_input_flags(cli.build_parser()).parse_args(["--input", "x", "--in-pix-fmt", "yuv444p"])
    assert not any(s.startswith("--in-") for act in cli.build_parser()._actions for s in act.option_strings if s != "--input")


def test_iter_yuv420_drops_a_trailing_partial_frame():
    import pythoncrt_amd as pc
    h, w = 5, 7
    fb = model.sizes(h, w)[2]
    data = np.random.default_rng(4).integers(0, 256, 3 * fb + fb // 2, dtype=np.uint8)

    class Dribble(io.BytesIO):                                  # a pipe may return less than asked for
        def read(self, n=-1):
            return super().read(min(n, 11) if n and n > 0 else n)
    for stream in (io.BytesIO(data.tobytes()), Dribble(data.tobytes())):
        frames = list(pc.iter_yuv420(stream, w, h))
        assert len(frames) == 3 and all(f.shape == (fb,) and f.dtype == np.uint8 for f in frames)
        assert np.array_equal(np.concatenate(frames), data[:3 * fb])
    assert list(pc.iter_yuv420(io.BytesIO(b""), w, h)) == []
