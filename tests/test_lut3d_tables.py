"""The 3D LUT stage without a GPU (include/crtfx_lut3d.h): the .cube reader and every refusal of it, the quantiser, the numpy model against
a float64 restatement, its independence of the order of equal fractions, identity cubes on every code, the half quantiser on all 65 536
patterns, the top edge; the C-ABI bound symbol for symbol and refusing bad arguments before it touches a device; the builds' registers and
the LDS boundary against the header; every refusal of process_frames(in_lut=, deliver_lut=) and of the CLIs' flags; the stages the two
chain ends build with and without the keywords.  A plan cannot exist without a device, so the refusals of crtfx_lut3d_set_table on a live
plan — another N, an entry above 1020, a null table — are held in tests/test_lut3d_gpu.py (test_set_cube_on_a_live_plan...); here only its
refusal of a null plan.  Tests write their .cube files themselves (lut3d_model.write_cube)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pythoncrt_amd import _lib, _stage, canvas, cube, depth, ends, formats, ingest, lut3d, resample, resize16  # noqa: E402
from pythoncrt_amd.cube import Cube  # noqa: E402
from tests import lut3d_model as model  # noqa: E402
from tests import resize16_model  # noqa: E402

HEADER = os.path.join(ROOT, "include", "crtfx_lut3d.h")

CUBE2 = """# a written-out 2 x 2 x 2 cube: red fastest
TITLE "two"

LUT_3D_SIZE 2
DOMAIN_MIN 0.0 0.0 0.0
DOMAIN_MAX 1.0 1.0 1.0
0 0 0
1 0 0.25
0 1 0
1 1 0
   # a comment between the rows
0 0 1
1 0 1
0 1 1
1.5 -0.5 0.5
"""


# ---- the reader ---------------------------------------------------------------------------------------------------------------------------

def test_a_written_out_cube_is_read_red_fastest(tmp_path):
    path = tmp_path / "two.cube"
    path.write_text(CUBE2)
    c = Cube.load(path)
    assert c.size == 2 and c.title == "two" and c.values.shape == (2, 2, 2, 3) and c.values.dtype == np.float64
    assert c.values[0, 0, 1].tolist() == [1.0, 0.0, 0.25]                     # [b][g][r]: the second row is r = 1
    assert c.values[0, 1, 0].tolist() == [0.0, 1.0, 0.0] and c.values[1, 0, 0].tolist() == [0.0, 0.0, 1.0]
    assert c.values[1, 1, 1].tolist() == [1.5, -0.5, 0.5]
    q = c.quantise()
    assert q.dtype == np.uint16 and q.shape == (2, 2, 2, 3)
    assert q[0, 0, 1].tolist() == [1020, 0, 255] and q[1, 1, 1].tolist() == [1020, 0, 510]      # clipped to 0..1
    # without the optional lines, and through parse / str paths / Cube objects
    bare = Cube.parse(["LUT_3D_SIZE 2"] + ["0.5 0.5 0.5"] * 8)
    assert bare.title == "" and (bare.quantise() == 510).all()
    assert cube.as_cube(str(path)).size == 2 and cube.as_cube(c) is c
    back = tmp_path / "back.cube"
    model.write_cube(back, c.values, c.title)
    assert np.array_equal(Cube.load(back).values, c.values)


def test_identity_and_the_constructor():
    for n in (2, 3, 17, 65):
        c = Cube.identity(n)
        assert c.size == n and np.array_equal(c.quantise(), model.identity_table(n))
        assert c.values[0, 0, n - 1].tolist() == [1.0, 0.0, 0.0] and c.values[n - 1, 0, 0].tolist() == [0.0, 0.0, 1.0]
    assert Cube(2, np.zeros(24)).values.shape == (2, 2, 2, 3)
    for bad in (1, 66, 0, -2, 2.5, True):
        with pytest.raises(ValueError, match="2..65"):
            Cube(bad, np.zeros(24))
        with pytest.raises(ValueError, match="2..65"):
            Cube.identity(bad)
    with pytest.raises(ValueError, match="8 rows"):
        Cube(2, np.zeros(21))
    with pytest.raises(ValueError, match="finite"):
        Cube(2, np.full(24, np.nan))
    for bad in (7, None, b"x", ["a"]):
        with pytest.raises(ValueError, match="a path to a .cube file or a Cube"):
            cube.as_cube(bad, "in_lut")
    with pytest.raises(ValueError, match="in_lut=.*cannot read"):
        cube.as_cube("/nonexistent/dir/x.cube", "in_lut")


ROWS8 = ["0 0 0"] * 8
REFUSALS = [
    (["LUT_1D_SIZE 16"] + ROWS8, 1, "LUT_1D_SIZE"),
    (["TITLE \"x\"", "LUT_3D_SIZE 2", "DOMAIN_MIN 0 0 0.1"] + ROWS8, 3, "DOMAIN_MIN"),
    (["LUT_3D_SIZE 2", "", "DOMAIN_MAX 1 1 2"] + ROWS8, 3, "DOMAIN_MAX"),
    (["LUT_3D_SIZE 2", "DOMAIN_MAX 1 1"] + ROWS8, 2, "DOMAIN_MAX"),
    (["LUT_3D_SIZE 1", "0 0 0"], 1, "outside 2..65"),
    (["# c", "LUT_3D_SIZE 66"], 2, "outside 2..65"),
    (["LUT_3D_SIZE two"], 1, "not an integer"),
    (["LUT_3D_SIZE 2"] + ROWS8[:7], 8, "7 of the 8 rows"),
    (["LUT_3D_SIZE 2"] + ROWS8 + ["0 0 0"], 10, "more than the 8 rows"),
    (["LUT_3D_SIZE 2"] + ROWS8[:3] + ["0 nan 0"] + ROWS8[:4], 5, "non-finite"),
    (["LUT_3D_SIZE 2"] + ROWS8[:3] + ["inf 0 0"] + ROWS8[:4], 5, "non-finite"),
    (["LUT_3D_SIZE 2", "LUT_3D_INPUT_RANGE 0 1"] + ROWS8, 2, "unknown keyword LUT_3D_INPUT_RANGE"),
    (["LUT_3D_SIZE 2", "LUT_IN_VIDEO_RANGE"] + ROWS8, 2, "unknown keyword"),
    (["LUT_3D_SIZE 2"] + ROWS8[:2] + ["0 0"] + ROWS8[:5], 4, "three values"),
    (["LUT_3D_SIZE 2"] + ROWS8[:2] + ["0 0 x"] + ROWS8[:5], 4, "not a row of three numbers"),
    (["0 0 0", "LUT_3D_SIZE 2"], 1, "in front of LUT_3D_SIZE"),
    (["LUT_3D_SIZE 2", "LUT_3D_SIZE 2"] + ROWS8, 2, "second LUT_3D_SIZE"),
    (["LUT_3D_SIZE 2"] + ROWS8[:4] + ["TITLE late"] + ROWS8[:4], 6, "behind the table"),
]


@pytest.mark.parametrize("lines,line_no,word", REFUSALS, ids=[r[2].replace(" ", "_") + f"@{r[1]}" for r in REFUSALS])
def test_the_reader_refuses_with_the_line(tmp_path, lines, line_no, word):
    path = tmp_path / "bad.cube"
    path.write_text("\n".join(lines) + "\n")
    with pytest.raises(ValueError) as e:
        Cube.load(path)
    assert f"bad.cube, line {line_no}:" in str(e.value) and word in str(e.value), str(e.value)


def test_a_file_without_a_size_is_refused(tmp_path):
    path = tmp_path / "empty.cube"
    path.write_text("# nothing\nTITLE \"t\"\n")
    with pytest.raises(ValueError, match="empty.cube: no LUT_3D_SIZE"):
        Cube.load(path)


# ---- the quantiser ----------------------------------------------------------------------------------------------------------------------------

def test_quantiser_clips_and_rounds_ties_to_even():
    v = np.array([0.0, 1.0, -0.0, -3.0, 2.0, 1e-12, 0.5 / 1020, 1.5 / 1020, 2.5 / 1020, 1019.5 / 1020, 0.25, 1.0 - 1e-12])
    exp = [0, 1020, 0, 0, 1020, 0, 0, 2, 2, 1020, 255, 1020]
    assert (1020.0 * v[6:9] == [0.5, 1.5, 2.5]).all()                          # the products are the ties themselves
    got = model.quantise_cube(v)
    assert got.dtype == np.uint16 and got.tolist() == exp
    c = Cube(2, np.resize(v, 24))
    assert c.quantise().ravel()[:12].tolist() == exp and c.quantise().max() <= _lib.LUT3D_QMAX == model.QMAX == 1020


# ---- the model --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [255, 1020])
@pytest.mark.parametrize("n", [2, 5, 17, 33, 65])
def test_model_against_the_float_restatement(n, S):
    """sum / 1020 against exact tetrahedral interpolation of the same table in float64.  The integer sum IS 1020 x the interpolant of the
    integer table at x / S up to float64's own rounding (S * float = sum exactly in the rationals: the weights are the fractions times S), so
    |S * float - sum| is bounded by the float evaluation's error, a few ulps of 1020 * S; and out = (sum + 510) // 1020 is the interpolant
    scaled by S / 1020 and rounded to nearest: within half a unit of it, so within one unit."""
    t = model.random_table(n, seed=S)
    px = model.pixels(np.uint8 if S == 255 else np.float16, 6000, seed=n)
    x = px.astype(np.int64) if S == 255 else resize16_model.quantise(px)
    out, total = model.apply_codes(x, t, S)
    fl = model.apply_float(x, t, S)                                           # on the table's 0..1020 scale
    assert np.abs(S * fl - total).max() <= 1e-6
    assert np.abs(out - fl * S / 1020.0).max() <= 0.5 + 1e-9
    assert out.min() >= 0 and out.max() <= S


@pytest.mark.parametrize("n", [2, 5, 17, 33])
def test_tie_order_independence(n):
    t = model.random_table(n, seed=1)
    for dtype in (np.uint8, np.float16):
        px = model.pixels(dtype, 4096, seed=n)
        S = 255 if dtype == np.uint8 else 1020
        x = px.astype(np.int64) if dtype == np.uint8 else resize16_model.quantise(px)
        # forced ties: two and three channels on one cell fraction, the corners among them
        ties = x.copy()
        ties[::2, 1] = ties[::2, 0]
        ties[::4, 2] = ties[::4, 0]
        _, f = model.split(ties, n, S)
        assert (f[:, 0] == f[:, 1]).sum() >= 2048 and ((f[:, 0] == f[:, 1]) & (f[:, 1] == f[:, 2])).sum() >= 1024
        for codes in (x, ties):
            ref = model.apply_codes(codes, t, S, "stable")[0]
            for order in model.ORDERS[1:]:
                assert np.array_equal(model.apply_codes(codes, t, S, order)[0], ref), (n, dtype, order)


def test_tie_orders_differ_as_orders():
    f = np.array([[5, 5, 5], [3, 3, 1], [1, 3, 3]])
    perms = [model._perm(f, o).tolist() for o in model.ORDERS]
    assert perms[0][0] == [0, 1, 2] and perms[1][0] == [2, 1, 0] and perms[2][0] == [2, 0, 1]
    assert perms[0][1] == [0, 1, 2] and perms[1][1] == [1, 0, 2]


@pytest.mark.parametrize("n", model.IDENTITY_SIZES)
def test_identity_cubes_are_exact_on_every_code(n):
    t = model.identity_table(n)
    assert np.array_equal(t, Cube.identity(n).quantise())
    rng = np.random.default_rng(n)
    u = np.arange(256, dtype=np.uint8)
    for frame in (np.stack([u, u, u], -1), np.stack([u, rng.permutation(u), rng.permutation(u)], -1), np.stack([rng.permutation(u), u[::-1], u], -1)):
        assert np.array_equal(model.apply(frame, t), frame), n
    q = np.arange(1021)
    for codes in (np.stack([q, q, q], -1), np.stack([q, rng.permutation(q), rng.permutation(q)], -1), np.stack([rng.permutation(q), q[::-1], q], -1)):
        assert np.array_equal(model.apply_codes(codes, t, 1020)[0], codes), n
        halves = resize16_model.to_half(codes)
        assert np.array_equal(model.apply(halves, t).view(np.uint16), halves.view(np.uint16)), n


def test_all_half_patterns_go_through_the_quantiser():
    halves = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    q = resize16_model.quantise(halves)
    assert q.min() == 0 and q.max() == 1020
    f = halves.astype(np.float64)
    nan = np.isnan(f)
    assert (q[nan] == 0).all() and (q[f <= 0] == 0).all() and (q[np.isposinf(f)] == 1020).all() and (q[f >= 255] == 1020).all()
    inside = ~nan & (f > 0) & (f < 255)
    assert np.array_equal(q[inside], np.rint(4 * f[inside]).astype(np.int64))
    # every pattern in one channel beside random others, through an identity cube: the quarter code of each comes back
    rng = np.random.default_rng(5)
    for c in range(3):
        px = (rng.integers(0, 1021, (65536, 3)) / 4.0).astype(np.float16)
        px[:, c] = halves
        out = model.apply(px, model.identity_table(33))
        assert np.array_equal(out.astype(np.float64) * 4, resize16_model.quantise(px))


@pytest.mark.parametrize("S", [255, 1020])
def test_the_top_edge_in_each_channel(S):
    """x = S: num = S (N - 1), i = N - 2 (the min), f = S — the pixel sits on the far face of the last cell, and the entry read is T[N - 1]."""
    for n in (2, 3, 33, 65):
        t = model.random_table(n, seed=9)
        for c in range(3):
            x = np.zeros((1, 3), dtype=np.int64)
            x[0, c] = S
            i, f = model.split(x, n, S)
            assert i[0, c] == n - 2 and f[0, c] == S and i[0, c - 1] == 0 and f[0, c - 1] == 0
            p = [0, 0, 0]
            p[c] = n - 1
            exp = (S * t[p[2], p[1], p[0]].astype(np.int64) + 510) // 1020
            assert np.array_equal(model.apply_codes(x, t, S)[0][0], exp)
        x = np.full((1, 3), S)
        assert np.array_equal(model.apply_codes(x, t, S)[0][0], (S * t[n - 1, n - 1, n - 1].astype(np.int64) + 510) // 1020)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------------------

_vp = ctypes.c_void_p
_u16p = ctypes.POINTER(ctypes.c_uint16)
SIGNATURES = {
    "crtfx_lut3d_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _u16p, ctypes.POINTER(_vp)]),
    "crtfx_lut3d_destroy": (ctypes.c_int, [_vp]),
    "crtfx_lut3d_last_error": (ctypes.c_char_p, [_vp]),
    "crtfx_lut3d_run": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
    "crtfx_lut3d_set_table": (ctypes.c_int, [_vp, ctypes.c_int, _u16p]),
    "crtfx_lut3d_set_option": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "crtfx_lut3d_last_plan": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t]),
}


def test_symbols_are_bound_and_the_header_declares_them():
    assert _lib.LUT3D_SYMBOLS == SIGNATURES and (_lib.LUT3D_OPT_FORCE_GENERAL, _lib.LUT3D_OPT_FORCE_GLOBAL) == (1, 2)
    lib = _lib.load()
    for name, (res, args) in SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    hdr = open(HEADER).read()
    for text in ("CRTFX_LUT3D_OPT_FORCE_GENERAL = 1", "CRTFX_LUT3D_OPT_FORCE_GLOBAL = 2", "#define CRTFX_LUT3D_QMAX 1020", "#define CRTFX_LUT3D_MIN_N 2",
                 "#define CRTFX_LUT3D_MAX_N 65", "#define CRTFX_LUT3D_LDS_MAX_N 34", "#define CRTFX_LUT3D_LDS_BYTES 163840"):
        assert text in hdr, text
    assert (_lib.LUT3D_QMAX, _lib.LUT3D_MIN_N, _lib.LUT3D_MAX_N, _lib.LUT3D_LDS_MAX_N) == (1020, 2, 65, 34) == (cube.QMAX, cube.MIN_N, cube.MAX_N, 34)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_lut3d_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(SIGNATURES) and len(protos) == 7, set(protos) ^ set(SIGNATURES)
    for name, args in protos.items():
        assert len(args.split(",")) == len(SIGNATURES[name][1]), name
    order = [a.split()[-1].lstrip("*") for a in protos["crtfx_lut3d_create"].split(",")]
    assert order == ["device", "h", "w", "pix_fmt", "N", "table", "out_plan"]
    assert [a.split()[-1].lstrip("*") for a in protos["crtfx_lut3d_set_table"].split(",")] == ["plan", "N", "table"]
    others = set()
    for table in ("SYMBOLS", "INGEST_SYMBOLS", "EGRESS_SYMBOLS", "UNPACK_SYMBOLS", "DEEP_SYMBOLS", "YUV422_SYMBOLS", "DEEP444_SYMBOLS", "SITED_SYMBOLS",
                  "EGRESS_SITED_SYMBOLS", "RESIZE16_SYMBOLS", "RESAMPLE_SYMBOLS", "CANVAS_SYMBOLS", "DEPTH_SYMBOLS", "DEINT_SYMBOLS"):
        others |= set(getattr(_lib, table))
    assert not set(SIGNATURES) & others
    assert all(os.path.basename(f) in {os.path.basename(s) for s in _lib.SOURCES} for f in ("crtfx_lut3d.hip", "crtfx_lut3d.h"))
    assert all(os.path.exists(s) for s in _lib.SOURCES) and "crtfx_lut3d" in _lib.STAGE_UNITS
    import pythoncrt_amd as pc
    assert pc.Lut3D is lut3d.Lut3D and pc.Cube is Cube and "Lut3D" in pc.__all__ and "Cube" in pc.__all__ and issubclass(pc.Lut3D, _stage.Handle)
    import bench                                                               # a namespace of its own, outside the chain's evidence hash
    assert "crtfx_lut3d" not in open(bench.__file__).read()
    assert "namespace crtfx_lut3d_impl" in open(os.path.join(_lib.CSRC, "crtfx_lut3d.hip")).read()


def _table(n=3, fill=0):
    return (ctypes.c_uint16 * (n ** 3 * 3))(*([fill] * (n ** 3 * 3)))


GOOD = dict(device=0, h=9, w=24, pix_fmt=_lib.PIX_U8, N=3)


def _create(lib, no_out=False, table="good", **kw):
    a = dict(GOOD)
    a.update(kw)
    plan = ctypes.c_void_p(1)
    tab = _table(max(2, min(65, a["N"]))) if isinstance(table, str) else table
    rc = lib.crtfx_lut3d_create(*(a[k] for k in GOOD), tab, None if no_out else ctypes.byref(plan))
    return rc, plan, (lib.crtfx_lut3d_last_error(None) or b"").decode()


def test_create_refuses_bad_arguments_before_it_touches_a_device():
    """Every refusal of crtfx_lut3d_create comes before the device is asked for, so it holds on any machine; *out_plan is NULL and the
    message names the offending field."""
    lib = _lib.load()
    cases = [({k: v}, k + " =") for k in ("h", "w") for v in (0, -3, 32768)]
    cases += [(dict(N=v), "N =") for v in (1, 0, -1, 66, 1000)]
    cases += [(dict(pix_fmt=v), "pix_fmt") for v in (2, -1, 7)]
    for kw, word in cases:
        rc, plan, msg = _create(lib, **kw)
        assert rc == _lib.E_INVALID and not plan.value and word in msg, (kw, rc, plan.value, msg)
    rc, plan, msg = _create(lib, table=None)
    assert rc == _lib.E_INVALID and not plan.value and "table is null" in msg
    for pos in (0, 40, 80):
        tab = _table(3)
        tab[pos] = 1021
        rc, plan, msg = _create(lib, table=tab)
        assert rc == _lib.E_INVALID and not plan.value and f"entry {pos} = 1021" in msg and "1020" in msg, msg
    tab = _table(3, 1020)
    tab[80] = 65535
    rc, plan, msg = _create(lib, table=tab)
    assert rc == _lib.E_INVALID and "entry 80 = 65535" in msg
    rc, plan, msg = _create(lib, no_out=True)
    assert rc == _lib.E_INVALID and "out_plan" in msg
    import torch
    if not torch.cuda.is_available():                                          # what is admitted passes every check: what is left to fail is the device
        for kw in (dict(), dict(pix_fmt=_lib.PIX_F16), dict(N=2), dict(N=65), dict(h=1, w=1), dict(h=32767, w=32767), dict(table=_table(3, 1020))):
            rc, plan, msg = _create(lib, **kw)
            assert rc == _lib.E_HIP and not plan.value and "device" in msg.lower(), (kw, rc, msg)
    else:
        rc, plan, msg = _create(lib, device=4096)
        assert rc == _lib.E_HIP and not plan.value and "4096" in msg
    assert lib.crtfx_lut3d_destroy(None) == _lib.OK and lib.crtfx_lut3d_set_option(None, 1, 1) == _lib.E_INVALID
    assert lib.crtfx_lut3d_set_table(None, 3, _table(3)) == _lib.E_INVALID
    assert lib.crtfx_lut3d_run(None, None, 0, None, 0, 1, None) == _lib.E_INVALID
    assert lib.crtfx_lut3d_last_plan(None, ctypes.create_string_buffer(8), 8) == _lib.E_INVALID


def test_python_plan_refuses_before_a_device(tmp_path):
    import torch
    with pytest.raises(ValueError, match="ROCm device"):
        lut3d.Lut3D("cpu", (4, 4), Cube.identity(2))
    with pytest.raises(ValueError, match="dtype"):
        lut3d.Lut3D("cpu", (4, 4), Cube.identity(2), dtype=torch.float32)
    with pytest.raises(ValueError, match="cannot read"):
        lut3d.Lut3D("cpu", (4, 4), str(tmp_path / "missing.cube"))
    bad = tmp_path / "bad.cube"
    bad.write_text("LUT_1D_SIZE 4\n")
    with pytest.raises(ValueError, match="line 1"):
        lut3d.Lut3D("cpu", (4, 4), str(bad))


# what include/crtfx_lut3d.h states for the eight builds: VGPRs as built
HEADER_VGPRS = {"k_lut3d<u8,lds,vec>": 30, "k_lut3d<u8,lds,general>": 28, "k_lut3d<u8,global,vec>": 42, "k_lut3d<u8,global,general>": 29,
                "k_lut3d<half,lds,vec>": 55, "k_lut3d<half,lds,general>": 28, "k_lut3d<half,global,vec>": 55, "k_lut3d<half,global,general>": 29}


def test_lut3d_kernels_hold_the_register_budget_and_the_header():
    """Registers, LDS and scratch of the eight builds, read from the built library's code objects (tools/kernel_resources.py): at most 64
    VGPRs + AGPRs (two blocks of 1024 lanes per CU), blocks of 1024 lanes, no static LDS, no scratch memory, no spills — and the figures the
    header quotes are the figures of this build."""
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {re.sub(r"crtfx_lut3d_impl::", "", n).replace(", ", ","): v for n, v in res.items() if n.startswith("crtfx_lut3d_impl::")}
    assert set(found) == set(HEADER_VGPRS), sorted(found)
    hdr = open(HEADER).read()
    for name, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == 0 and v["vgpr_count"] + v["agpr_count"] <= 64 and v["agpr_count"] == 0, (name, v)
        assert v["max_flat_workgroup_size"] == 1024, (name, v)
        assert v["vgpr_count"] == HEADER_VGPRS[name], (name, v["vgpr_count"])
        assert re.search(rf"{re.escape(name)} {HEADER_VGPRS[name]}\b", hdr), name
    assert "no AGPRs, no static LDS" in hdr and "no scratch, no spills" in hdr


def test_the_lds_boundary_is_the_headers():
    """34^3 dwords fit a CU's LDS and 35^3 do not; 33 takes the 143 748 bytes the plan string reports; a cube of N >= 28 leaves room for
    one block per CU."""
    hdr = open(HEADER).read()
    lds = int(re.search(r"#define CRTFX_LUT3D_LDS_BYTES (\d+)", hdr).group(1))
    top = int(re.search(r"#define CRTFX_LUT3D_LDS_MAX_N (\d+)", hdr).group(1))
    assert lds == 160 * 1024 and top == 34
    assert 4 * top ** 3 == 157216 <= lds < 4 * (top + 1) ** 3 == 171500 and 4 * 33 ** 3 == 143748
    assert lds // (4 * 27 ** 3) == 2 and lds // (4 * 28 ** 3) == 1
    for text in ("157 216", "171 500", "143 748", "163 840", "N >= 28"):
        assert text in hdr, text
    src = open(os.path.join(_lib.CSRC, "crtfx_lut3d.hip")).read()
    assert "N <= CRTFX_LUT3D_LDS_MAX_N" in src and "CRTFX_LUT3D_LDS_BYTES / p->lds_bytes" in src


def test_the_default_table_path_follows_the_measured_run():
    """profiles/lut3d.txt is the one run the header's timing block and README's row quote: every figure of it stands in the header, lds is
    the faster table path for N = 17 and 33 at both sizes on both sample types, and so the plan takes lds for every N it holds."""
    txt = open(os.path.join(ROOT, "profiles", "lut3d.txt")).read()
    rows = re.findall(r"^(1080p|4K)\s+(uint8|float16)\s+N=\s*(\d+) k_lut3d<\w+,(lds|global),(vec|general)>\s+([\d.]+) us/frame", txt, re.M)
    assert len(rows) == 2 * 2 * (4 + 4 + 2), len(rows)
    copies = re.findall(r"device-to-device copy of equal traffic\s+([\d.]+) us/frame", txt)
    assert len(copies) == 12
    hdr, readme = open(HEADER).read(), open(os.path.join(ROOT, "README.md")).read()
    assert "profiles/lut3d.txt" in hdr and "profiles/lut3d.txt" in readme and "tools/lut3d_kernel_times.py" in hdr
    us = {(size, dt, int(n), table, walk): v for size, dt, n, table, walk, v in rows}
    for key, v in us.items():
        assert re.search(rf"(?<![\d.]){re.escape(v)}(?![\d])", hdr), (key, v)
        if key[4] == "vec":                                                    # README's row quotes the vec walk
            assert re.search(rf"(?<![\d.]){re.escape(v)}(?![\d])", readme), (key, v)
    for n in (17, 33):
        for size in ("1080p", "4K"):
            for dt in ("uint8", "float16"):
                assert float(us[(size, dt, n, "lds", "vec")]) < float(us[(size, dt, n, "global", "vec")]), (n, size, dt)
    assert not any(k[3] == "lds" for k in us if k[2] == 65)
    src = open(os.path.join(_lib.CSRC, "crtfx_lut3d.hip")).read()
    assert "bool lds_default(int N) { return N <= CRTFX_LUT3D_LDS_MAX_N; }" in src
    assert "default for every N it holds" in hdr


# ---- process_frames and the CLI: every refusal comes before a device --------------------------------------------------------------------------

def _refusing_process_frames(monkeypatch):
    import torch
    import pythoncrt_amd as pc

    def never():
        raise AssertionError("a frame was read")
        yield

    def no_device():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    return lambda **kw: pc.process_frames(never(), lambda a: None, 80, 46, 30.0, 1, **kw)


def _files(tmp_path):
    good = tmp_path / "good.cube"
    model.write_cube(good, Cube.identity(2).values)
    bad = tmp_path / "bad.cube"
    bad.write_text("LUT_3D_SIZE 2\n0 0 0\nDOMAIN_MIN 0 0 0\n")
    return str(good), str(bad), str(tmp_path / "missing.cube")


def test_process_frames_refusals(tmp_path, monkeypatch):
    run = _refusing_process_frames(monkeypatch)
    good, bad, missing = _files(tmp_path)
    for key in ("in_lut", "deliver_lut"):
        with pytest.raises(ValueError, match=f"{key}=.*missing.cube.*cannot read"):
            run(**{key: missing})
        with pytest.raises(ValueError, match="bad.cube, line 3: keyword DOMAIN_MIN behind the table"):
            run(**{key: bad})
        for value in (5, 1.5, b"x.cube", ("a",)):
            with pytest.raises(ValueError, match=f"{key} must be a path to a .cube file or a Cube"):
                run(**{key: value})
    with pytest.raises(ValueError, match="resize_on='host' cannot be combined with in_lut"):
        run(in_lut=good, resize_on="host")
    with pytest.raises(ValueError, match="resize_on='host' cannot be combined with in_lut"):
        run(in_lut=Cube.identity(3), resize_on="host")
    # what is admitted: the next thing asked for is the device
    for kw in (dict(in_lut=good), dict(deliver_lut=good), dict(in_lut=Cube.identity(65), deliver_lut=good), dict(deliver_lut=good, resize_on="host"),
               dict(in_lut=good, chain_pix="half", dither="ordered"), dict(in_lut=good, in_pix_fmt="p010le", out_pix_fmt="x2rgb10le"),
               dict(in_lut=good, in_pix_fmt="nv12", in_size=(50, 90)), dict(deliver_lut=good, deliver_size=(36, 64), deliver_fit="pad")):
        with pytest.raises(AssertionError, match="the device was asked for"):
            run(**kw)


def test_cli_flags_refusals_and_the_sharded_cli(tmp_path, monkeypatch):
    from pythoncrt_amd import cli
    good, bad, missing = _files(tmp_path)
    src = tmp_path / "in.rgb"
    src.write_bytes(bytes(46 * 80 * 3))
    out = tmp_path / "out.rgb"
    base = ["--input", str(src), "--output", str(out), "--width", "80", "--height", "46"]

    def refused(extra, *words):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code not in (0, None) and all(w in str(e.value) for w in words), (extra, str(e.value))
        assert not out.exists()
    for flag in ("--in-lut", "--deliver-lut"):
        refused([flag, missing], flag, "missing.cube", "cannot read")
        refused([flag, bad], flag, "bad.cube, line 3")
        with pytest.raises(SystemExit):                                         # argparse: the flag takes a file
            cli.main(base + [flag])
    # the flags live in add_input_flags / add_output_flags, not in the reference's schema
    assert not any(act.dest in ("in_lut", "deliver_lut") for act in cli.build_parser()._actions)
    a = cli.add_input_flags(cli.add_output_flags(cli.build_parser())).parse_args(base)
    assert (a.in_lut, a.deliver_lut) == ("", "") and cli.luts_from_args(a) == (None, None)
    spec, ranks = cli.check_flags(a)
    assert spec.deliver is None and spec.half is False and ranks is None
    a = cli.add_input_flags(cli.add_output_flags(cli.build_parser())).parse_args(base + ["--in-lut", good, "--deliver-lut", good])
    spec, ranks = cli.check_flags(a)
    assert spec.deliver is None and spec.half is False and ranks is None
    cubes = cli.luts_from_args(a)
    assert [c.size for c in cubes] == [2, 2] and cli.luts_from_args(a) is cubes      # read once
    monkeypatch.setenv("CRTFX_FORCE_DIST", "1")
    refused(["--in-lut", good], "--in-lut", "sharded CLI")
    refused(["--deliver-lut", good], "--deliver-lut", "sharded CLI")
    refused(["--in-lut", missing], "--in-lut", "sharded CLI")


# ---- which stages the chain ends build --------------------------------------------------------------------------------------------------------

RESIZES = (ingest.IngestResize, resize16.ResizeHalf, resample.Resample)
FORMAT_PLANS = sorted({f.source for f in formats.FORMATS.values()} | {f.egress for f in formats.FORMATS.values()}, key=lambda c: c.__name__)


@pytest.fixture
def built(monkeypatch):
    """Every plan class records (class name, positional arguments past the device, keywords) instead of creating its plan; a format plan
    still knows its frame_bytes, as StagePlan.__init__ sets it."""
    log = []
    for cls in list(RESIZES) + FORMAT_PLANS + [canvas.Canvas, depth.Widen, depth.Narrow, lut3d.Lut3D]:
        def init(self, *args, _cls=cls, **kw):
            log.append((_cls.__name__, args[1:], kw))
            if issubclass(_cls, _stage.StagePlan):
                self.frame_bytes = _cls._frame_bytes(args[1][0], args[1][1], kw["layout"])
        monkeypatch.setattr(cls, "__init__", init)
    return log


R, S, D = (24, 32), (48, 64), (12, 16)              # render, an off-size source, a delivery
NV12 = {"layout": "nv12", "matrix": "bt601", "range": "tv"}
P010 = {"layout": "p010le", "matrix": "bt601", "range": "tv"}
I420 = {"layout": "yuv420p", "matrix": "bt601", "range": "tv"}
X2 = {"layout": "x2rgb10le", "matrix": "bt601", "range": "tv"}


def test_source_end_stage_lists(built):
    import torch
    u8, f16 = torch.uint8, torch.float16
    c = Cube.identity(3)
    lut_u8, lut_f16 = ("Lut3D", (R, c), {"dtype": u8}), ("Lut3D", (R, c), {"dtype": f16})
    table = [
        # (format, source size, chain dtype, widen) -> the stages with the cube
        (("rgb24", R, u8, False), [lut_u8]),                                                     # the LUT is the only stage
        (("rgb24", S, u8, False), [("IngestResize", (S, R), {}), lut_u8]),
        (("nv12", S, u8, False), [("UnpackYuv", (S,), NV12), ("IngestResize", (S, R), {}), lut_u8]),
        (("rgb24", R, f16, True), [("Widen", (R,), {}), lut_f16]),                               # behind the Widen: the LUT sees halves
        (("nv12", S, f16, True), [("UnpackYuv", (S,), NV12), ("IngestResize", (S, R), {}), ("Widen", (R,), {}), lut_f16]),
        (("p010le", R, f16, False), [("UnpackYuv10", (R,), P010), lut_f16]),
    ]
    for (fmt, hw, pix, widen), want in table:
        del built[:]
        src = ends.SourceEnd("dev", R, fmt, "bt601", "tv", "replicate", hw, "bilinear", None, pix, widen=widen, lut=c)
        assert built == want, (fmt, hw, built)
        assert [type(st).__name__ for st, _ in src.stages] == [b[0] for b in want] and src.stages[-1][0] is src.lut and src.stages[-1][1] == R
        assert src.chain_dtype == pix and src.dtype == (f16 if fmt == "p010le" else u8)
        # ... and without it: the same list less the LUT, and no Lut3D is created
        del built[:]
        src = ends.SourceEnd("dev", R, fmt, "bt601", "tv", "replicate", hw, "bilinear", None, pix, widen=widen)
        assert built == want[:-1] and src.lut is None and [type(st).__name__ for st, _ in src.stages] == [b[0] for b in want[:-1]]
    # the buffers between the stages: the Widen's output, read by the LUT, is a half buffer; the others keep the source side's dtype
    del built[:]
    src = ends.SourceEnd("cpu", R, "rgb24", "bt601", "tv", "replicate", S, "bilinear", None, f16, widen=True, lut=c)
    src.slots(2, 2, pinned=False)
    assert [type(st).__name__ for st, _ in src.stages] == ["IngestResize", "Widen", "Lut3D"]
    assert [m[0].dtype for m in src.mid] == [u8, f16] and [tuple(m[0].shape) for m in src.mid] == [(2,) + R + (3,)] * 2


def test_delivery_end_stage_lists(built):
    import torch
    u8, f16 = torch.uint8, torch.float16
    c = Cube.identity(3)
    table = [
        (("rgb24", u8, None, None), []),
        (("rgb24", u8, D, None), [("IngestResize", (R, D), {})]),
        (("yuv420p", u8, D, None), [("IngestResize", (R, D), {}), ("EgressYuv", (D,), I420)]),
        (("yuv420p", f16, D, "ordered"), [("ResizeHalf", (R, D), {}), ("Narrow", (D,), {"dither": "ordered"}), ("EgressYuv", (D,), I420)]),
        (("x2rgb10le", f16, None, None), [("EgressDeep444", (R,), X2)]),
        (("rgb24", f16, None, "none"), [("Narrow", (R,), {"dither": "none"})]),
    ]
    for (fmt, pix, deliver, narrow), want in table:
        del built[:]
        end = ends.DeliveryEnd("dev", R, pix, fmt, "bt601", "tv", "center", deliver, "bilinear", narrow=narrow, lut=c)
        assert built == [("Lut3D", (R, c), {"dtype": pix})] + want, (fmt, built)      # the first stage, at render size, on the chain's pixels
        assert end.stages[0] == (end.lut, R) and len(end.stages) == 1 + len([b for b in want if not b[0].startswith("Egress")])
        del built[:]
        end = ends.DeliveryEnd("dev", R, pix, fmt, "bt601", "tv", "center", deliver, "bilinear", narrow=narrow)
        assert built == want and end.lut is None
    # a pad: the Canvas and its colour stand behind the LUT, the Narrow and its dither stay last
    del built[:]
    end = ends.DeliveryEnd("dev", (48, 64), f16, "nv12", "bt601", "tv", "center", (36, 64), "bilinear", deliver_fit="pad", pad_color=(7, 200, 33),
                           narrow="ordered", lut=c)
    assert built == [("Lut3D", ((48, 64), c), {"dtype": f16}), ("ResizeHalf", ((48, 64), (36, 48)), {}),
                     ("Canvas", ((36, 48), (36, 64)), {"at": (0, 8), "fill": (7, 200, 33), "dtype": f16}),
                     ("Narrow", ((36, 64),), {"dither": "ordered"}), ("EgressYuv", ((36, 64),), {"layout": "nv12", "matrix": "bt601", "range": "tv"})]
    assert [hw for _, hw in end.stages] == [(48, 64), (36, 48), (36, 64), (36, 64)]
