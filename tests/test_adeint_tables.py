"""The motion-adaptive deinterlace stage without a GPU (include/crtfx_adeint.h): the model against a per-pixel restatement of the header and
against the properties that follow from the rule (EDGE without a previous frame, the weave where nothing changed, EDGE where everything
did, between e and c everywhere, BOTH against FIRST, chained single frames, every half pattern, a field-rate scene against its progressive
truth), the C-ABI bound symbol for symbol and refusing bad arguments before it touches a device, every refusal of
process_frames(deinterlace="adaptive") and of the CLIs, the stages SourceEnd builds, and the builds' registers against the header."""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pythoncrt_amd import _lib, _stage, adeint, canvas, deint, depth, ends, formats, ingest, resample, resize16  # noqa: E402
from tests import adeint_model as model  # noqa: E402
from tests import deint_model as dm  # noqa: E402

HEADER = os.path.join(ROOT, "include", "crtfx_adeint.h")
DTYPES = (np.uint8, np.float16)
COMBOS = list(itertools.product(model.ORDERS, model.FIELDS))


# ---- the arithmetic -------------------------------------------------------------------------------------------------------------------------

def _loop_frame(C, P, field):
    """One output frame, pixel by pixel, as the header states it.  C, P: [h, w, 3] frames (P may be None)."""
    h, w = C.shape[:2]
    c = dm.codes(C).tolist()
    p = dm.codes(P).tolist() if P is not None else None
    out = C.copy()
    for y in range(h):
        if y % 2 == field:
            continue
        ya, yb = (y - 1 if y > 0 else y + 1), (y + 1 if y < h - 1 else y - 1)
        two = y > 0 and y < h - 1
        a, b = c[ya], c[yb]
        for x in range(w):
            d = 0
            if two and 3 <= x <= w - 4:
                def S(j):
                    return sum(abs(a[x + t + j][k] - b[x + t - j][k]) for t in (-1, 0, 1) for k in range(3))
                s = S(0) - 1
                for j in (-1, 1):
                    if S(j) < s:
                        s, d = S(j), j
                        if S(2 * j) < s:
                            s, d = S(2 * j), 2 * j
            e = [(a[x + d][k] + b[x - d][k] + 1) >> 1 for k in range(3)]
            if p is None:
                r = e
            else:
                t0 = max(abs(c[y][x][k] - p[y][x][k]) for k in range(3))
                if two:
                    t1 = max((abs(c[y - 1][x][k] - p[y - 1][x][k]) + abs(c[y + 1][x][k] - p[y + 1][x][k]) + 1) >> 1 for k in range(3))
                else:
                    t1 = max(abs(c[ya][x][k] - p[ya][x][k]) for k in range(3))
                m = max(t0, t1)
                r = [min(max(e[k], c[y][x][k] - m), c[y][x][k] + m) for k in range(3)]
            out[y, x] = dm.from_codes(np.array(r, dtype=np.int64), C.dtype.type)
    return out


def _loop(frames, prev, order, fields):
    first = model.ORDERS.index(order)
    outs = []
    for i, C in enumerate(frames):
        P = prev if i == 0 else frames[i - 1]
        for field in ((first,) if fields == "first" else (first, 1 - first)):
            outs.append(_loop_frame(C, P, field))
    return np.stack(outs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", [(2, 1), (3, 7), (5, 9), (6, 12)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_model_is_the_headers_rule_pixel_by_pixel(size, dtype):
    frames, prev = model.scene(3, size[0], size[1], dtype, seed=size[0] * 100 + size[1])
    for order, fields in COMBOS:
        for pv in (None, prev):
            assert np.array_equal(dm.bits(model.adaptive(frames, pv, order, fields)), dm.bits(_loop(frames, pv, order, fields))), (order, fields, pv is None)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order,fields", COMBOS)
def test_without_a_previous_frame_it_is_edge(dtype, order, fields):
    for h, w in ((2, 1), (3, 8), (23, 40)):
        src = dm.noise(h, w, n=1, dtype=dtype, seed=h)
        assert np.array_equal(dm.bits(model.adaptive(src, None, order, fields)), dm.bits(dm.deinterlace(src, "edge", order, fields)))
    # ... and only frame 0 of a batch has none
    src = dm.noise(9, 12, n=3, dtype=dtype, seed=4)
    per = 2 if fields == "both" else 1
    got, edge = model.adaptive(src, None, order, fields), dm.deinterlace(src, "edge", order, fields)
    assert np.array_equal(dm.bits(got[:per]), dm.bits(edge[:per])) and not np.array_equal(dm.bits(got[per:]), dm.bits(edge[per:]))


@pytest.mark.parametrize("order,fields", COMBOS)
def test_a_still_picture_is_woven(order, fields):
    per = 2 if fields == "both" else 1
    src = dm.noise(9, 16, n=1, dtype=np.uint8, seed=8)
    still = np.repeat(src, 3, axis=0)
    assert np.array_equal(model.adaptive(still, src[0], order, fields), np.repeat(still, per, axis=0))      # uint8: the source frames themselves
    half = dm.noise(9, 16, n=1, dtype=np.float16, seed=8).copy()
    half.view(np.uint16)[0, :, :4, :] = np.array([0x7e01, 0xfc01, 0x8000, 0xc500, 0x7bff, 0x0001, 0x7c00, 0xfe55, 0x3555, 0x5bf9, 0x5c01, 0x7fff],
                                                 dtype=np.uint16).reshape(4, 3)
    out = model.adaptive(np.repeat(half, 2, axis=0), half[0], order, fields)
    first = model.ORDERS.index(order)
    for j in range(out.shape[0]):
        f = first if fields == "first" or j % per == 0 else 1 - first
        assert np.array_equal(dm.bits(out[j, f::2]), dm.bits(half[0, f::2]))                                # kept: bits, NaN payloads included
        assert np.array_equal(dm.bits(out[j, 1 - f::2]), dm.bits(dm.from_codes(dm.codes(half[0, 1 - f::2]), np.float16)))   # made: the dequantised codes


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order,fields", COMBOS)
def test_a_wholly_changed_picture_is_edge(dtype, order, fields):
    """C with codes in 96..159 against an all-zero P: m >= 96 > 63 >= |e - c|."""
    rng = np.random.default_rng(6)
    c = rng.integers(96, 160, (2, 11, 24, 3))
    src = dm.from_codes(c, dtype)
    assert dm.codes(src).min() >= 96 and dm.codes(src).max() <= 159
    zero = np.zeros((11, 24, 3), dtype=dtype)
    got = model.adaptive(src[:1], zero, order, fields)
    assert np.array_equal(dm.bits(got), dm.bits(dm.deinterlace(src[:1], "edge", order, fields)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_made_sample_lies_between_e_and_c_and_both_sides_of_the_clamp_occur(dtype):
    frames, prev = model.scene(4, 23, 40, dtype, seed=2)
    for order, fields in COMBOS:
        out, parts = model.adaptive_parts(frames, prev, order, fields)
        per = len(parts)
        for j, (e, c, m, ys) in enumerate(parts):
            r = dm.codes(out[j::per][:, ys])
            assert ((r >= np.minimum(e, c)) & (r <= np.maximum(e, c))).all()
            gap = np.abs(e - c)
            assert (m[..., None] == 0).any() and ((m[..., None] > 0) & (m[..., None] < gap)).any() and (m[..., None] >= gap).any()
            assert np.array_equal(r[np.broadcast_to(m[..., None] == 0, r.shape)], c[np.broadcast_to(m[..., None] == 0, r.shape)])
            assert np.array_equal(r[m[..., None] >= gap], e[m[..., None] >= gap])


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_is_first_of_the_two_orders_and_batches_chain(dtype):
    frames, prev = model.scene(4, 10, 17, dtype, seed=9)
    for pv in (None, prev):
        t, b = model.adaptive(frames, pv, "tff", "first"), model.adaptive(frames, pv, "bff", "first")
        both_t, both_b = model.adaptive(frames, pv, "tff", "both"), model.adaptive(frames, pv, "bff", "both")
        assert np.array_equal(dm.bits(both_t[0::2]), dm.bits(t)) and np.array_equal(dm.bits(both_t[1::2]), dm.bits(b))
        assert np.array_equal(dm.bits(both_b[0::2]), dm.bits(b)) and np.array_equal(dm.bits(both_b[1::2]), dm.bits(t))
        # each output frame depends on frames i - 1 and i only: the single-frame calls chained
        for order, fields in COMBOS:
            whole = model.adaptive(frames, pv, order, fields)
            chained = np.concatenate([model.adaptive(frames[i:i + 1], pv if i == 0 else frames[i - 1], order, fields) for i in range(len(frames))])
            assert np.array_equal(dm.bits(whole), dm.bits(chained))
    assert model.adaptive(frames[:0], prev, "tff", "both").shape == (0, 10, 17, 3)


def test_every_half_pattern_through_c_and_p_on_a_made_row():
    w = 65536 // 3 + 1
    pats = np.arange(65536, dtype=np.uint16)
    C = dm.noise(3, w, 1, np.float16, seed=1).copy()
    P = dm.noise(3, w, 1, np.float16, seed=2)[0].copy()
    C.view(np.uint16)[0, 1].reshape(-1)[:65536] = pats
    P.view(np.uint16)[1].reshape(-1)[:65536] = np.roll(pats, 12345)
    out, parts = model.adaptive_parts(C, P, "tff", "first")
    e, c, m, ys = parts[0]
    assert list(ys) == [1]
    r = out[0, 1].astype(np.float64) * 4
    assert np.array_equal(r, np.rint(r)) and r.min() >= 0 and r.max() <= 1020
    assert ((r >= np.minimum(e, c)[0, 0]) & (r <= np.maximum(e, c)[0, 0])).all()
    lo = slice(0, 64)                                                           # ... and the rule itself on a stretch of them, pixel by pixel
    assert np.array_equal(dm.bits(model.adaptive(C[:, :, lo], P[:, lo], "tff", "first")), dm.bits(_loop(C[:, :, lo], P[:, lo], "tff", "first")))
    # the same patterns in both: m = 0 on that row wherever the neighbours agree too, and the sample is the dequantised pattern
    P2 = C[0].copy()
    same = model.adaptive(C, P2, "tff", "first")
    assert np.array_equal(dm.bits(same[0, 1]), dm.bits(dm.from_codes(dm.codes(C[0, 1]), np.float16)))


def test_a_field_rate_scene_is_woven_where_it_stands_still():
    """A still noise background with a block that moves 2 pixels per field, woven into frames and deinterlaced to both fields: on every pixel
    whose rows y - 1, y, y + 1 the block touches in neither frame of the pair, the adaptive output IS the progressive truth and EDGE's is not."""
    h, w, bh, bw, nf = 32, 48, 8, 8, 4
    back = dm.noise(h, w, 1, np.uint8, seed=21)[0]
    block = dm.noise(bh, bw, 1, np.uint8, seed=22)[0]
    truth, cover = [], []
    for k in range(2 * nf):                                                     # one progressive frame per FIELD
        t, cv = back.copy(), np.zeros((h, w), dtype=bool)
        x0 = 4 + 2 * k
        t[12:12 + bh, x0:x0 + bw] = block
        cv[12:12 + bh, x0:x0 + bw] = True
        truth.append(t)
        cover.append(cv)
    truth = np.stack(truth)
    for order in model.ORDERS:
        first = model.ORDERS.index(order)
        woven = np.empty((nf, h, w, 3), dtype=np.uint8)
        woven[:, first::2] = truth[0::2, first::2]
        woven[:, 1 - first::2] = truth[1::2, 1 - first::2]
        got = model.adaptive(woven, None, order, "both")
        edge = dm.deinterlace(woven, "edge", order, "both")
        bad_a = bad_e = quiet_px = 0
        for i in range(1, nf):                                                  # frame 0 has no previous frame
            touched = cover[2 * i - 2] | cover[2 * i - 1] | cover[2 * i] | cover[2 * i + 1]
            near = touched.copy()
            near[1:] |= touched[:-1]
            near[:-1] |= touched[1:]
            quiet = ~near
            assert quiet.mean() >= 0.5
            for j in (0, 1):
                quiet_px += int(quiet.sum())
                bad_a += int((got[2 * i + j][quiet] != truth[2 * i + j][quiet]).sum())
                bad_e += int((edge[2 * i + j][quiet] != truth[2 * i + j][quiet]).sum())
        assert bad_a == 0 and bad_e > quiet_px // 4, (bad_a, bad_e, quiet_px)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------------------

_vp = ctypes.c_void_p
SIGNATURES = {
    "crtfx_adeint_create": (ctypes.c_int, [ctypes.c_int] * 6 + [ctypes.POINTER(_vp)]),
    "crtfx_adeint_destroy": (ctypes.c_int, [_vp]),
    "crtfx_adeint_last_error": (ctypes.c_char_p, [_vp]),
    "crtfx_adeint_frames_out": (ctypes.c_int, [_vp]),
    "crtfx_adeint_run": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
    "crtfx_adeint_set_option": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "crtfx_adeint_last_plan": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t]),
}


def test_symbols_are_bound_and_the_header_declares_them():
    assert _lib.ADEINT_SYMBOLS == SIGNATURES and _lib.ADEINT_OPT_FORCE_GENERAL == 1
    lib = _lib.load()
    for name, (res, args) in SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    hdr = open(HEADER).read()
    for text in ("CRTFX_ADEINT_OPT_FORCE_GENERAL = 1", "NOT claimed is equality with any other deinterlacer", "yadif", "bwdif",
                 "no clamp to the code range is needed", "crtfx_edge.hip.h", "adeint=k_adeint<u8,both,vec>;frames=5"):
        assert text in hdr, text
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(crtfx_adeint_\w+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(SIGNATURES) and len(protos) == 7, set(protos) ^ set(SIGNATURES)
    for name, args in protos.items():
        assert len(args.split(",")) == len(SIGNATURES[name][1]), name
    assert [a.split()[-1].lstrip("*") for a in protos["crtfx_adeint_create"].split(",")] == ["device", "h", "w", "pix_fmt", "order", "fields", "out_plan"]
    assert [a.split()[-1].lstrip("*") for a in protos["crtfx_adeint_run"].split(",")] == [
        "plan", "prev_frame", "src_base", "src_stride_bytes", "dst_base", "dst_stride_bytes", "n", "stream"]
    others = set()
    for table in ("SYMBOLS", "INGEST_SYMBOLS", "EGRESS_SYMBOLS", "UNPACK_SYMBOLS", "DEEP_SYMBOLS", "YUV422_SYMBOLS", "DEEP444_SYMBOLS", "SITED_SYMBOLS",
                  "EGRESS_SITED_SYMBOLS", "RESIZE16_SYMBOLS", "RESAMPLE_SYMBOLS", "CANVAS_SYMBOLS", "DEPTH_SYMBOLS", "DEINT_SYMBOLS", "LUT3D_SYMBOLS"):
        others |= set(getattr(_lib, table))
    assert not set(SIGNATURES) & others
    names = {os.path.basename(s) for s in _lib.SOURCES}
    assert {"crtfx_adeint.hip", "crtfx_adeint.h", "crtfx_edge.hip.h"} <= names and all(os.path.exists(s) for s in _lib.SOURCES)
    assert "crtfx_adeint" in _lib.STAGE_UNITS
    import pythoncrt_amd as pc
    assert pc.AdaptiveDeinterlace is adeint.AdaptiveDeinterlace and "AdaptiveDeinterlace" in pc.__all__ and issubclass(pc.AdaptiveDeinterlace, _stage.Handle)
    assert adeint.METHOD == "adaptive" and deint.METHODS == ("linear", "edge")
    import bench                                                               # a namespace of its own, outside the chain's evidence hash
    assert "adeint" not in open(bench.__file__).read()
    unit = open(os.path.join(_lib.CSRC, "crtfx_adeint.hip")).read()
    assert "namespace crtfx_adeint_impl" in unit and '#include "crtfx_edge.hip.h"' in unit and "edge_search" in unit
    assert '#include "crtfx_edge.hip.h"' in open(os.path.join(_lib.CSRC, "crtfx_deint.hip")).read()      # shared, not restated
    assert unit.count("void edge_search") == 0


GOOD = dict(device=0, h=9, w=24, pix_fmt=_lib.PIX_U8, order=_lib.DEINT_BFF, fields=_lib.DEINT_BOTH)


def _create(lib, no_out=False, **kw):
    a = dict(GOOD)
    a.update(kw)
    plan = ctypes.c_void_p(1)
    rc = lib.crtfx_adeint_create(*(a[k] for k in GOOD), None if no_out else ctypes.byref(plan))
    return rc, plan, (lib.crtfx_adeint_last_error(None) or b"").decode()


def test_create_refuses_bad_arguments_before_it_touches_a_device():
    lib = _lib.load()
    cases = [(dict(h=v), "h =") for v in (1, 0, -3, 32768)] + [(dict(w=v), "w =") for v in (0, -3, 32768)]
    cases += [({k: v}, k) for k in ("pix_fmt", "order", "fields") for v in (2, -1, 7)]
    for kw, word in cases:
        rc, plan, msg = _create(lib, **kw)
        assert rc == _lib.E_INVALID and not plan.value and word in msg, (kw, rc, plan.value, msg)
    rc, plan, msg = _create(lib, no_out=True)
    assert rc == _lib.E_INVALID and "out_plan" in msg
    for kw in (dict(), dict(h=2, w=1), dict(h=32767, w=32767, pix_fmt=_lib.PIX_F16), dict(order=0, fields=0)):
        rc, plan, msg = _create(lib, device=4096, **kw)
        assert rc == _lib.E_HIP and not plan.value and "no HIP device 4096" in msg, (kw, rc, msg)
    assert lib.crtfx_adeint_destroy(None) == _lib.OK and lib.crtfx_adeint_set_option(None, 1, 1) == _lib.E_INVALID
    assert lib.crtfx_adeint_frames_out(None) == 0
    assert lib.crtfx_adeint_run(None, None, None, 0, None, 0, 1, None) == _lib.E_INVALID
    assert lib.crtfx_adeint_last_plan(None, ctypes.create_string_buffer(8), 8) == _lib.E_INVALID


def test_python_plan_refuses_before_a_device():
    for kw in (dict(order="top"), dict(fields="second"), dict(fields=2)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            adeint.AdaptiveDeinterlace("cpu", (4, 4), **kw)
    with pytest.raises(ValueError, match="ROCm device"):
        adeint.AdaptiveDeinterlace("cpu", (4, 4))
    with pytest.raises(TypeError):
        adeint.AdaptiveDeinterlace("cpu", (4, 4), method="edge")


# what include/crtfx_adeint.h states for the eight builds: VGPRs as built
HEADER_VGPRS = {
    "k_adeint<u8,first,vec>": 126, "k_adeint<u8,both,vec>": 128, "k_adeint<f16,first,vec>": 148, "k_adeint<f16,both,vec>": 150,
    "k_adeint<u8,first,general>": 63, "k_adeint<u8,both,general>": 63, "k_adeint<f16,first,general>": 66, "k_adeint<f16,both,general>": 64}


def test_adeint_kernels_have_no_scratch_and_the_headers_registers():
    import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    res = kernel_resources.resources(_lib.LIB_PATH)
    found = {n.replace("crtfx_adeint_impl::", "").replace("crtfx_deint_impl::", "").replace(", ", ","): v
             for n, v in res.items() if n.startswith("crtfx_adeint_impl::")}
    assert set(found) == set(HEADER_VGPRS), sorted(found)
    hdr = open(HEADER).read()
    for name, v in found.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] == 0 and v["agpr_count"] == 0, (name, v)
        assert v["vgpr_count"] == HEADER_VGPRS[name], (name, v["vgpr_count"])
        assert re.search(rf"{re.escape(name)} {HEADER_VGPRS[name]}\b", hdr), name
    assert "no AGPRs, no LDS, no scratch, no spills" in hdr
    # the family beside it is untouched: exactly its sixteen kernels
    old = [n for n in res if n.startswith("crtfx_deint_impl::")]
    assert len(old) == 16 and all("k_deint<" in n for n in old), sorted(old)


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


def test_process_frames_refusals(monkeypatch):
    import pythoncrt_amd as pc
    run = _refusing_process_frames(monkeypatch)
    for bad in ("Adaptive", "adaptive ", "yadif", "bwdif"):
        with pytest.raises(ValueError, match="deinterlace must be 'off' or one of linear, edge, adaptive"):
            run(deinterlace=bad)
    for bad in ("top", "", None):
        with pytest.raises(ValueError, match="field_order must be"):
            run(deinterlace="adaptive", field_order=bad)
    for bad in ("second", "", 2):
        with pytest.raises(ValueError, match="deinterlace_fields must be"):
            run(deinterlace="adaptive", deinterlace_fields=bad)
    with pytest.raises(ValueError, match="resize_on='host' cannot be combined with deinterlace='adaptive'"):
        run(deinterlace="adaptive", resize_on="host")
    for kw in (dict(in_size=(1, 80)), dict(in_size=(1, 80), in_pix_fmt="nv12"), dict(in_size=(0, 80), in_pix_fmt="uyvy422")):
        with pytest.raises(ValueError, match="deinterlace='adaptive': a source frame of . row\\(s\\) has no two fields"):
            run(deinterlace="adaptive", **kw)
    with pytest.raises(ValueError, match="no two fields"):
        pc.process_frames(iter(()), lambda a: None, 80, 1, 30.0, 1, deinterlace="adaptive", in_pix_fmt="uyvy422")
    for kw in (dict(deinterlace="adaptive"), dict(deinterlace="adaptive", field_order="bff", deinterlace_fields="both"),
               dict(deinterlace="adaptive", in_pix_fmt="nv12", in_size=(50, 90)), dict(deinterlace="adaptive", in_pix_fmt="p010le", out_pix_fmt="yuv420p10le"),
               dict(deinterlace="adaptive", in_crop=(3, 0, 20, 40)), dict(deinterlace="adaptive", chain_pix="half", deinterlace_fields="both")):
        with pytest.raises(AssertionError, match="the device was asked for"):
            run(**kw)


def test_cli_refusals_and_the_sharded_cli(tmp_path, monkeypatch):
    from pythoncrt_amd import cli
    src = tmp_path / "in.rgb"
    src.write_bytes(bytes(46 * 80 * 3))
    out = tmp_path / "out.rgb"
    base = ["--input", str(src), "--output", str(out), "--width", "80", "--height", "46"]

    def refused(extra, *words, args=base):
        with pytest.raises(SystemExit) as e:
            cli.main(args + extra)
        assert e.value.code not in (0, None) and all(w in str(e.value) for w in words), (extra, str(e.value))
        assert not out.exists()
    one_row = ["--input", str(src), "--output", str(out), "--width", "80", "--height", "1"]
    refused(["--deinterlace", "adaptive"], "--deinterlace adaptive", "no two fields", args=one_row)
    refused(["--field-order", "bff"], "nothing to deinterlace", "adaptive")
    parse = cli.add_input_flags(cli.add_output_flags(cli.build_parser())).parse_args
    a = parse(base + ["--deinterlace", "adaptive"])
    spec, ranks = cli.check_flags(a)
    assert spec.deinterlace == ("adaptive", "tff", "first") and spec.deliver is None and spec.half is False and ranks is None
    a = parse(base + ["--deinterlace", "adaptive", "--field-order", "bff", "--deinterlace-fields", "both"])
    spec, ranks = cli.check_flags(a)
    assert spec.deinterlace == ("adaptive", "bff", "both") and spec.deliver is None and spec.half is False and ranks is None
    assert "--deinterlace adaptive" in cli.__doc__ and "crtfx_adeint.h" in cli.__doc__
    monkeypatch.setenv("CRTFX_FORCE_DIST", "1")
    refused(["--deinterlace", "adaptive"], "sharded CLI", "--deinterlace")
    refused(["--deinterlace", "adaptive", "--deinterlace-fields", "both"], "sharded CLI", "--deinterlace")


# ---- which stages SourceEnd builds ------------------------------------------------------------------------------------------------------------

RESIZES = (ingest.IngestResize, resize16.ResizeHalf, resample.Resample)


@pytest.fixture
def built(monkeypatch):
    """Canvas, the resize plans, Widen and the two deinterlacers record (class, positional arguments, keywords) instead of creating a plan."""
    log = []
    for cls in RESIZES + (canvas.Canvas, depth.Widen, deint.Deinterlace, adeint.AdaptiveDeinterlace):
        def init(self, *args, _cls=cls, **kw):
            log.append((_cls, args, kw))
        monkeypatch.setattr(cls, "__init__", init)
    return log


def test_source_end_stages(built, monkeypatch):
    import torch
    u8, f16 = torch.uint8, torch.float16
    A = adeint.AdaptiveDeinterlace

    class Plan:
        frame_bytes = 123
    monkeypatch.setattr(formats, "source_plan", lambda *a: None if a[2] == "rgb24" else Plan())
    R, S = (24, 32), (48, 64)
    for fields, ratio in (("first", 1), ("both", 2)):
        del built[:]
        src = ends.SourceEnd("dev", R, "rgb24", "bt601", "tv", "replicate", R, "bilinear", deinterlace=("adaptive", "bff", fields))
        assert built == [(A, ("dev", R), {"order": "bff", "fields": fields, "dtype": u8})]
        assert [hw for _, hw in src.stages] == [R] and src.stages[0][0] is src.deint and src.ratio == ratio and src.adaptive
    del built[:]
    src = ends.SourceEnd("dev", R, "nv12", "bt601", "tv", "replicate", S, "bilinear", (6, 0, 36, 64), deinterlace=("adaptive", "tff", "both"))
    assert built == [(A, ("dev", S), {"order": "tff", "fields": "both", "dtype": u8}),
                     (canvas.Canvas, ("dev", S, (36, 64)), {"window": (6, 0, 36, 64), "dtype": u8}), (ingest.IngestResize, ("dev", (36, 64), R), {})]
    assert [type(st) for st, _ in src.stages] == [Plan, A, canvas.Canvas, ingest.IngestResize]
    assert [hw for _, hw in src.stages] == [S, S, (36, 64), R] and src.ratio == 2 and src.frame_shape == (123,)
    del built[:]
    src = ends.SourceEnd("dev", R, "p010le", "bt601", "tv", "replicate", R, "bilinear", None, f16, deinterlace=("adaptive", "tff", "first"))
    assert built == [(A, ("dev", R), {"order": "tff", "fields": "first", "dtype": f16})] and src.ratio == 1
    del built[:]
    src = ends.SourceEnd("dev", R, "rgb24", "bt601", "tv", "replicate", S, "bilinear", None, f16, widen=True, deinterlace=("adaptive", "bff", "both"))
    assert [b[0] for b in built] == [A, ingest.IngestResize, depth.Widen] and built[0][2]["dtype"] == u8 and built[0][1] == ("dev", S)
    # every other configuration: no AdaptiveDeinterlace, and restart() does nothing
    for kw in (dict(), dict(deinterlace=None), dict(deinterlace=("edge", "tff", "both")), dict(deinterlace=("linear", "bff", "first"))):
        del built[:]
        src = ends.SourceEnd("dev", R, "nv12", "bt601", "tv", "replicate", S, "bilinear", **kw)
        assert not any(b[0] is A for b in built) and not src.adaptive
        if src.deint is not None:
            src.deint.reset = lambda: pytest.fail("restart() reached a Deinterlace")
        assert src.restart() is None


def test_source_end_pushes_and_restarts(built, monkeypatch):
    """slots(B) as under the Deinterlace; convert(d, n, dst) calls push() on the adaptive plan and run() on every other stage; restart() is
    its reset()."""
    import torch

    class Plan:
        frame_bytes = 123
    monkeypatch.setattr(formats, "source_plan", lambda *a: Plan())
    shapes = []
    real_empty = torch.empty

    def empty(shape, dtype=None, device=None):
        shapes.append((tuple(shape), device))
        return real_empty(shape, dtype=dtype)
    monkeypatch.setattr(torch, "empty", empty)
    src = ends.SourceEnd("dev", (24, 32), "nv12", "bt601", "tv", "replicate", (48, 64), "bilinear", deinterlace=("adaptive", "tff", "both"))
    src.slots(4, 2, pinned=False)
    assert [s for s, dev in shapes if dev == "dev"] == [(4, 48, 64, 3)] * 2 + [(8, 48, 64, 3)] * 2 + [(4, 123)] * 2
    calls = []
    for st, _ in src.stages:
        word = "push" if st is src.deint else "run"
        other = "run" if st is src.deint else "push"
        setattr(st, word, lambda x, out, _st=st, _w=word: calls.append((type(_st), _w, tuple(x.shape), tuple(out.shape))) or out)
        setattr(st, other, lambda *a, **k: pytest.fail("the wrong entry point"))
    src.deint.reset = lambda: calls.append("reset")
    dst = real_empty((6, 24, 32, 3), dtype=torch.uint8)
    src.convert(1, 3, dst)
    src.restart()
    assert calls == [(Plan, "run", (3, 123), (3, 48, 64, 3)), (adeint.AdaptiveDeinterlace, "push", (3, 48, 64, 3), (6, 48, 64, 3)),
                     (ingest.IngestResize, "run", (6, 48, 64, 3), (6, 24, 32, 3)), "reset"]
