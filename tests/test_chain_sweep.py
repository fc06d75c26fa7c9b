"""The sweep of the whole chain, its host part (tests/chain_model.py; the device part is tests/test_chain_sweep_gpu.py): every seeded draw
and explicit case is admitted by options.refuse — none is skipped —, the cases together reach every format, stage kind and pair of kinds,
the composer's wiring is the one ends.py builds (plan classes patched to record, no device), and the composer itself returns the bytes
of three expectations written out by hand from the stage models."""
import itertools
from collections import Counter

import numpy as np
import pytest

from pythoncrt_amd import (adeint, canvas, deint, depth, formats, ingest, interlace, lut3d, options, resample, resize16, sited,
                           tables)
from pythoncrt_amd import signal as signal_mod
from tests import (adeint_model, canvas_model, deep444_model, deep_model, deint_model, depth_model, egress_sited_model, interlace_model,
                   lut3d_model, resample_model, resize16_model, signal_model, sited_model, yuv_model)
from tests import chain_model as cm

CASES = cm.cases()
EVERY = CASES + list(cm.STREAMS)


def _id(case):
    return case["id"]


def test_the_draw_is_seeded_and_there_are_48():
    assert cm.N_DRAWS == 48 and len(cm.draws()) == 48 and cm.draw(7) == cm.draw(7) and len({c["id"] for c in EVERY}) == len(EVERY)


@pytest.mark.parametrize("case", EVERY, ids=_id)
def test_every_case_is_admitted(case):
    """A refusal is a failure of the generator: zero are allowed, and nothing is skipped."""
    options.refuse(cm.raw(case), "keywords")
    spec = options.ChainOptions.build(cm.raw(case), "keywords")
    d = cm.Derived(case)
    assert spec.resize_on == "device" and (spec.half, spec.widen, spec.narrow, spec.ratio) == (d.half, d.widen, d.narrow, d.ratio)
    assert spec.batch(case["batch"]) == (d.B, d.Bs) and spec.direct == d.direct and (spec.weave is not None) == d.weave
    assert 5 <= len(case["sizes"]) <= 13 and case["batch"] in (2, 3, 4) and len(cm.batches(case)) >= 2
    assert all(s[0] <= 48 and s[1] <= 72 for s in case["sizes"])


# ---- what the cases reach ---------------------------------------------------------------------------------------------------------------------------

def test_every_format_on_both_ends():
    assert {c["kw"]["in_pix_fmt"] for c in CASES} == set(formats.PIX_FMTS) == {c["kw"]["out_pix_fmt"] for c in CASES}


def test_every_value_of_every_domain():
    seen = lambda key, where=lambda kw: True: {c["kw"][key] for c in CASES if where(c["kw"])}       # noqa: E731
    assert seen("in_chroma") == {"replicate", "left", "center"} and seen("out_chroma") == {"center", "left"}
    assert seen("in_chroma_rows") == {"progressive", "interlaced"}
    assert {c["kw"]["in_filter"] for c in CASES if "source resize" in cm.kinds(c)} == set(tables.RESAMPLE_FILTERS)
    assert {c["kw"]["deliver_filter"] for c in CASES if "delivery resize" in cm.kinds(c)} == set(tables.RESAMPLE_FILTERS)
    on = lambda kw: kw["deinterlace"] != "off"       # noqa: E731
    assert seen("deinterlace") == {"off", "linear", "edge", "adaptive"}
    assert {(kw["field_order"], kw["deinterlace_fields"]) for kw in (c["kw"] for c in CASES) if on(kw)} == set(itertools.product(("tff", "bff"), ("first", "both")))
    cable = lambda kw: kw["in_signal"] != "rgb"       # noqa: E731
    assert seen("in_signal") == {"rgb", "composite", "svideo"} and seen("signal_chroma", cable) == {"sharp", "soft"} and seen("signal_crawl", cable) == {True, False}
    for key in ("in_cube", "deliver_cube"):
        assert {None if c[key] is None else c[key][0] for c in CASES} == {None, 17, 33}, key
    assert {(c["kw"]["chain_pix"], c["kw"]["dither"]) for c in CASES} == {("auto", "none"), ("half", "none"), ("half", "ordered")}
    assert set(depth.DITHERS) == {"none", "ordered"}
    assert {(c["kw"]["deliver_interlace"], c["kw"]["deliver_lowpass"]) for c in CASES} >= set(itertools.product(("tff", "bff"), interlace_model.LOWPASS)) | {("off", "none")}
    for key in ("in_matrix", "out_matrix"):
        assert {(c["kw"][key], c["kw"][key.replace("matrix", "range")]) for c in CASES} == set(itertools.product(cm.MATRICES, cm.RANGES)), key
    area = lambda s: s[0] * s[1]       # noqa: E731
    for c in CASES:
        assert c["kw"]["in_crop"] is None or (c["kw"]["in_crop"][0] % 2 == 1 and c["kw"]["in_crop"][1] % 2 == 1), c["id"]
        assert c["kw"]["deliver_fit"] != "pad" or c["kw"]["deliver_pad_color"] != (0, 0, 0), c["id"]
    assert {np.sign(area(c["sizes"][0]) - area(c["render"])) for c in CASES} == {-1, 0, 1}
    fits = {(c["kw"]["deliver_fit"], int(np.sign(area(c["kw"]["deliver_size"]) - area(c["render"])))) for c in CASES if c["kw"]["deliver_size"] is not None}
    assert fits == set(itertools.product(("stretch", "pad", "crop"), (-1, 1)))
    assert {c["render"] for c in CASES} == set(cm.RENDERS)


def test_every_stage_kind_and_every_pair_of_kinds():
    count = Counter(k for c in CASES for k in cm.kinds(c))
    assert set(count) == set(cm.KINDS) and len(cm.KINDS) == 16
    assert all(count[k] >= 6 for k in cm.KINDS), count
    met = {frozenset(p) for c in CASES for p in itertools.combinations(cm.kinds(c), 2)}
    missing = [p for p in itertools.combinations(cm.KINDS, 2) if p not in cm.EXCLUSIVE and frozenset(p) not in met]
    assert not missing, missing
    assert not any(frozenset(p) in met for p in cm.EXCLUSIVE)                    # and what cannot be built together never is
    full = [c for c in CASES if len(cm.kinds(c)) == 13]                           # one of each exclusive pair: both ends with every stage present
    assert len(full) >= 4, [len(cm.kinds(c)) for c in CASES]


def test_chain_types_batches_and_pairs():
    combos = {(d.pix, d.ratio, d.weave) for d in map(cm.Derived, CASES)}
    assert combos == set(itertools.product(("uint8", "float16"), (1, 2), (False, True)))
    partial = [c for c in CASES if cm.batches(c)[-1][1] < cm.Derived(c).Bs]
    assert len(partial) >= 12, len(partial)
    odd = [c for c in CASES if cm.Derived(c).ratio == 2 and cm.Derived(c).weave and c["batch"] % 2 == 1]
    assert len(odd) >= 4, len(odd)
    assert sum(len(set(c["sizes"])) > 1 for c in CASES) >= 2 and max(len(set(c["sizes"])) for c in cm.STREAMS) == 6


def test_batches_restate_the_render_loop():
    """Even and at least 2 where frames come or go in pairs, divided by the ratio, cut at a change of source size."""
    c = cm.STREAMS[0]
    assert cm.Derived(c).Bs == 1 and [n for _, n, _ in cm.batches(c)] == [1] * 13
    c = cm.STREAMS[2]
    assert [(lo, n) for lo, n, _ in cm.batches(c)] == [(0, 2), (2, 1), (3, 2), (5, 2)] and cm.delivered_count(c) == 4
    c = cm._case("x", (24, 40), [(24, 40)] * 7, 3, deinterlace="edge", deinterlace_fields="both")
    assert (cm.Derived(c).B, cm.Derived(c).Bs) == (2, 1)
    c = cm._case("x", (24, 40), [(24, 40)] * 7, 3, deliver_interlace="tff")
    assert (cm.Derived(c).B, cm.Derived(c).Bs) == (2, 2) and cm.delivered_count(c) == 4
    c = cm._case("x", (24, 40), [(24, 40)] * 7, 3)
    assert [n for _, n, _ in cm.batches(c)] == [3, 3, 1]


# ---- the composer's wiring is the one ends.py builds --------------------------------------------------------------------------------------------

RESIZES = (ingest.IngestResize, resize16.ResizeHalf, resample.Resample)
PLANS = RESIZES + (signal_mod.Signal, deint.Deinterlace, adeint.AdaptiveDeinterlace, canvas.Canvas, depth.Widen, depth.Narrow, lut3d.Lut3D,
                   interlace.Interlace)


class _Plan:
    def __init__(self, name, frame_bytes):
        self.name, self.frame_bytes = name, frame_bytes


@pytest.fixture
def built(monkeypatch):
    """Every plan class records (positional arguments, keywords) on the instance instead of creating a plan; formats.source_plan and
    egress_plan return a record of what they were asked for; torch.empty allocates on the host and logs (shape, dtype) of device buffers."""
    import torch
    for cls in PLANS:
        def init(self, *args, **kw):
            self.args, self.kw = args, kw
        monkeypatch.setattr(cls, "__init__", init)

    def source_plan(device, size, fmt, matrix, rng, chroma, rows="progressive"):
        if fmt == "rgb24":
            return None
        fam = "field420" if rows == "interlaced" else "sited" if chroma != "replicate" else cm.family_of(fmt)
        assert rows == "progressive" or fmt in ("yuv420p", "nv12", "yuv420p10le", "p010le")
        assert chroma == "replicate" or fmt in sited.LAYOUTS
        return _Plan("source:" + fam, formats.frame_bytes(size[0], size[1], fmt))

    def egress_plan(device, size, fmt, matrix, rng, chroma):
        if fmt == "rgb24":
            return None
        fam = "sited" if chroma != "center" else cm.family_of(fmt)
        return _Plan("egress:" + fam, formats.frame_bytes(size[0], size[1], fmt))
    monkeypatch.setattr(formats, "source_plan", source_plan)
    monkeypatch.setattr(formats, "egress_plan", egress_plan)
    shapes, real_empty = [], torch.empty

    def empty(shape, dtype=None, device=None):
        if device == "dev":
            shapes.append((tuple(shape), str(dtype).replace("torch.", "")))
        return real_empty(shape, dtype=dtype)
    monkeypatch.setattr(torch, "empty", empty)
    return shapes


def _name(stage, delivery):
    """The composer's name of a built stage, and the sample type it was built for (None where the class has one only)."""
    if isinstance(stage, _Plan):
        return stage.name, None
    dt = stage.kw.get("dtype")
    dt = None if dt is None else str(dt).replace("torch.", "")
    if isinstance(stage, RESIZES):
        return ("deliver_resize" if delivery else "resize"), {ingest.IngestResize: "uint8", resize16.ResizeHalf: "float16"}.get(type(stage), dt)
    if isinstance(stage, canvas.Canvas):
        return ("crop" if not delivery else "crop_canvas" if "window" in stage.kw else "pad"), dt
    return {signal_mod.Signal: "signal", deint.Deinterlace: "deinterlace", adeint.AdaptiveDeinterlace: "adaptive", depth.Widen: "widen",
            depth.Narrow: "narrow", lut3d.Lut3D: "deliver_lut" if delivery else "in_lut", interlace.Interlace: "interlace"}[type(stage)], dt


def _resize_class(dt, filter):     # noqa: A002
    return resample.Resample if filter != "bilinear" else ingest.IngestResize if dt == "uint8" else resize16.ResizeHalf


@pytest.mark.parametrize("case", EVERY, ids=_id)
def test_the_trace_is_the_wiring(case, built):
    """Kinds, sizes and sample types of SourceEnd.stages / DeliveryEnd.stages are those of the composer's stage lists, the resize plans are
    of the class whose model the composer runs, and slots() allocates the composer's frame counts for a full batch."""
    import torch
    kw, d = case["kw"], cm.Derived(case)
    spec = options.ChainOptions.build(cm.raw(case), "keywords")
    pix = torch.float16 if spec.half else torch.uint8
    assert str(pix) == "torch." + d.pix
    for hw in sorted(set(case["sizes"])):
        want = cm.source_stages(case, hw)
        if not want:
            assert spec.direct and hw == case["render"]
            continue
        src = spec.source_end("dev", hw, pix)
        got = [_name(st, False) + (size,) for st, size in src.stages]
        assert [(n, s) for n, _, s in got] == [(n, s) for n, s, _, _ in want], (hw, got, want)
        for (name, dt, _), (_, _, wdt, _), (st, _) in zip(got, want, src.stages):
            # a stage's own sample type: the Widen reads uint8 and the Lut3D behind it runs on the chain's; every other stage writes what it reads
            assert dt in (None, wdt), (name, dt, wdt)
            if name == "resize":
                assert type(st) is _resize_class(wdt, kw["in_filter"]) and st.kw.get("filter", "bilinear") == kw["in_filter"]
            if name == "signal":
                assert st.kw == {"signal": kw["in_signal"], "chroma": kw["signal_chroma"], "crawl": kw["signal_crawl"], "dtype": getattr(torch, wdt)}
            if name in ("deinterlace", "adaptive"):
                assert (st.kw["order"], st.kw["fields"], st.kw.get("method", "adaptive")) == (kw["field_order"], kw["deinterlace_fields"], kw["deinterlace"])
            if name == "crop":
                assert st.kw["window"] == tuple(kw["in_crop"]) and st.args[1:] == (hw, tuple(kw["in_crop"][2:]))
        assert src.ratio == d.ratio and str(src.chain_dtype) == "torch." + d.pix
        del built[:]
        src.slots(d.Bs, 2, pinned=False)
        frame_shape = hw + (3,) if kw["in_pix_fmt"] == "rgb24" else (formats.frame_bytes(hw[0], hw[1], kw["in_pix_fmt"]),)
        mids = [((d.Bs * per,) + size + (3,), dt) for _, size, dt, per in want[:-1]]
        assert built == [m for m in mids for _ in range(2)] + [((d.Bs,) + frame_shape, "uint8")] * 2, (hw, built, mids)
    end = spec.delivery_end("dev", pix)
    want = cm.delivery_stages(case)
    stages = [st for st, _ in end.stages] + ([end.egress] if end.egress is not None else [])
    got = [_name(st, True) for st in stages]
    assert [n for n, _ in got] == [n for n, _, _, _ in want] and [s for _, s in end.stages] == [s for n, s, _, _ in want if not n.startswith("egress:")]
    for (name, dt), (_, size, wdt, _), st in zip(got, want, stages):
        assert dt in (None, d.pix), (name, dt)                                   # the geometry, the cube and the weave run on the chain's type
        if name == "deliver_resize":
            assert type(st) is _resize_class(d.pix, kw["deliver_filter"]) and st.kw.get("filter", "bilinear") == kw["deliver_filter"]
        if name == "pad":
            assert st.kw["fill"] == tuple(kw["deliver_pad_color"]) and st.kw["at"] == cm.delivery_geometry(case)[2]
        if name == "crop_canvas":
            assert tuple(st.kw["window"]) == cm.delivery_geometry(case)[3]
        if name == "interlace":
            assert (st.kw["order"], st.kw["lowpass"]) == (kw["deliver_interlace"], kw["deliver_lowpass"])
        if name == "narrow":
            assert st.kw == {"dither": kw["dither"]} and st.args[1] == size
    assert end.size == cm.delivery_geometry(case)[4] and [end.frames(m) for m in range(6)] == [d.delivered(m) for m in range(6)]
    del built[:]
    end.slots([torch.empty((d.B,) + case["render"] + (3,), dtype=pix) for _ in range(2)])
    bufs = [((d.delivered(d.B) if woven else d.B,) + ((size + (3,)) if not name.startswith("egress:") else (formats.frame_bytes(size[0], size[1], kw["out_pix_fmt"]),)), dt)
            for name, size, dt, woven in want]
    assert built == [b for b in bufs for _ in range(2)], (built, bufs)


# ---- the composer, against three expectations written out by hand ---------------------------------------------------------------------------------

def _same(got, exp, what):
    assert len(got) == len(exp), (what, len(got), len(exp))
    for i, (g, e) in enumerate(zip(got, exp)):
        g, e = np.asarray(g), np.asarray(e)
        assert g.shape == e.shape and g.dtype == e.dtype and np.array_equal(deint_model.bits(g), deint_model.bits(e)), (what, i)


def test_composer_eight_bit_by_hand():
    """yuv420p 30 x 44, chroma sited left -> composite cable -> linear, both fields, bff -> window (1, 3, 27, 40) -> bicubic to 24 x 40 ->
    cube 17 | identity | cube 33 -> centred window of 15:31 -> lanczos to 15 x 31 -> tff weave, linear low-pass -> uyvy422 sited left.
    Requested batch 4: two source frames, four frames of the chain, two delivered frames per batch; five source frames."""
    case = cm._case("hand-8bit", (24, 40), [(30, 44)] * 5, 4, 31, (17, 401), (33, 402), in_pix_fmt="yuv420p", in_size=(30, 44), in_chroma="left",
                    in_matrix="bt709", in_range="pc", in_signal="composite", deinterlace="linear", field_order="bff", deinterlace_fields="both",
                    in_crop=(1, 3, 27, 40), in_filter="bicubic", out_pix_fmt="uyvy422", out_chroma="left", out_range="pc", deliver_size=(15, 31),
                    deliver_fit="crop", deliver_filter="lanczos", deliver_interlace="tff", deliver_lowpass="linear")
    options.refuse(cm.raw(case), "keywords")
    items = cm.frames(case)
    rgb = np.stack([sited_model.unpack(p, 30, 44, "yuv420p", "left", "bt709", "pc") for p in items])
    rgb = signal_model.signal(rgb, "composite", "sharp", True, index=0)         # one run of consecutive frames: frame i is frame i of the stream
    rgb = deint_model.deinterlace(rgb, "linear", "bff", "both")
    assert rgb.shape == (10, 30, 44, 3)
    rgb = rgb[:, 1:28, 3:43]
    rgb = np.stack([resample_model.resize_u8(f, 24, 40, "bicubic") for f in rgb])
    rgb = lut3d_model.apply(rgb, lut3d_model.random_table(17, 401))
    rgb = lut3d_model.apply(rgb, lut3d_model.random_table(33, 402))
    win = canvas_model.fit_crop((24, 40), (15, 31))
    assert win == (2, 0, 19, 40)
    rgb = np.stack([resample_model.resize_u8(f[2:21], 15, 31, "lanczos") for f in rgb])
    woven = [interlace_model.weave(rgb[a], rgb[b], "tff", "linear") for a, b in ((0, 1), (2, 3), (4, 5), (6, 7), (8, 9))]
    exp = [egress_sited_model.pack(f, "uyvy422", "left", "bt601", "pc") for f in woven]
    got, trace = cm.expect(case)
    _same(got, exp, "hand-8bit")
    assert [n for _, n, _ in cm.batches(case)] == [2, 2, 1] and [len(t[-1][3]) for t in trace] == [2, 2, 1]
    assert [s[0] for s in trace[0]] == ["source:sited", "signal", "deinterlace", "crop", "resize", "in_lut", "chain", "deliver_lut", "crop_canvas",
                                        "deliver_resize", "interlace", "egress:sited"]


def test_composer_ten_bit_by_hand():
    """p010le at 24 x 40 -> adaptive, first field, bff, one history over the five frames though the batches hold 2, 2 and 1 -> identity ->
    cube 33 -> bilinear to the inner 36 x 60 -> bars of (12, 34, 56) -> yuv444p10le."""
    case = cm._case("hand-10bit", (24, 40), [(24, 40)] * 5, 2, 32, None, (33, 403), in_pix_fmt="p010le", deinterlace="adaptive", field_order="bff",
                    out_pix_fmt="yuv444p10le", out_matrix="bt709", deliver_size=(36, 64), deliver_fit="pad", deliver_pad_color=(12, 34, 56))
    options.refuse(cm.raw(case), "keywords")
    rgb = np.stack([deep_model.unpack(p, 24, 40, "p010le") for p in cm.frames(case)])
    assert rgb.dtype == np.float16
    rgb = adeint_model.adaptive(rgb, None, "bff", "first")
    per_batch = np.concatenate([adeint_model.adaptive(rgb0, None, "bff", "first") for rgb0 in
                                np.split(np.stack([deep_model.unpack(p, 24, 40, "p010le") for p in cm.frames(case)]), [2, 4])])
    assert not np.array_equal(deint_model.bits(rgb), deint_model.bits(per_batch))      # the history across the batches is another picture
    rgb = lut3d_model.apply(rgb, lut3d_model.random_table(33, 403))
    assert canvas_model.fit_pad((24, 40), (36, 64)) == ((36, 60), (0, 2))
    rgb = resize16_model.resize(rgb, 36, 60)
    out = np.empty((5, 36, 64, 3), dtype=np.float16)
    out[...] = np.array([12, 34, 56], dtype=np.float16)
    out[:, :, 2:62] = rgb
    exp = [deep444_model.pack(f, "yuv444p10le", "bt709", "tv") for f in out]
    got, trace = cm.expect(case)
    _same(got, exp, "hand-10bit")
    assert [s[0] for s in trace[2]] == ["source:deep420", "adaptive", "chain", "deliver_lut", "deliver_resize", "pad", "egress:deep444"]
    assert all(s[2] == "float16" for s in trace[0][:-1]) and [len(t[0][3]) for t in trace] == [2, 2, 1]


def test_composer_half_chain_by_hand():
    """rgb24 on a half chain: three frames of 31 x 57 then two of 24 x 40, requested batch 3 taken as 2 for the weave: batches of 2, 1 and 2
    source frames.  S-video cable without crawl (frame i is frame i of the stream across the change of size) -> hamming to 24 x 40 where the
    size differs -> Widen | identity | bff weave with the complex low-pass, the odd third frame with itself -> ordered Narrow -> nv12."""
    case = cm._case("hand-half", (24, 40), [(31, 57)] * 3 + [(24, 40)] * 2, 3, 33, in_signal="svideo", signal_chroma="soft", signal_crawl=False,
                    in_filter="hamming", chain_pix="half", dither="ordered", out_pix_fmt="nv12", out_matrix="bt709", deliver_interlace="bff",
                    deliver_lowpass="complex")
    options.refuse(cm.raw(case), "keywords")
    items = cm.frames(case)
    big = signal_model.signal(np.stack(items[:3]), "svideo", "soft", False, index=0)
    small = signal_model.signal(np.stack(items[3:]), "svideo", "soft", False, index=3)
    big = np.stack([resample_model.resize_u8(f, 24, 40, "hamming") for f in big])
    half = depth_model.widen(np.concatenate([big, small]))
    woven = np.stack([interlace_model.weave(half[0], half[1], "bff", "complex"), interlace_model.weave(half[2], half[2], "bff", "complex"),
                      interlace_model.weave(half[3], half[4], "bff", "complex")])
    exp = [yuv_model.pack(f, "nv12", "bt709", "tv") for f in depth_model.narrow(woven, "ordered")]
    got, trace = cm.expect(case)
    _same(got, exp, "hand-half")
    assert [(lo, n) for lo, n, _ in cm.batches(case)] == [(0, 2), (2, 1), (3, 2)]
    assert [s[0] for s in trace[0]] == ["signal", "resize", "widen", "chain", "interlace", "narrow", "egress:yuv420"]
    assert [s[0] for s in trace[2]] == ["signal", "widen", "chain", "interlace", "narrow", "egress:yuv420"]
    # with crawl the index matters: the composer hands each batch the stream index of its first frame
    crawl = cm._case("hand-crawl", (24, 40), [(24, 40)] * 5, 3, 34, in_signal="composite")       # the phase has a period of two frames: batches at 0 and 3
    exp = signal_model.signal(np.stack(cm.frames(crawl)), "composite", "sharp", True, index=0)
    _same(cm.expect(crawl)[0], list(exp), "hand-crawl")
    assert not np.array_equal(exp[3:5], signal_model.signal(np.stack(cm.frames(crawl)[3:5]), "composite", "sharp", True, index=0))
