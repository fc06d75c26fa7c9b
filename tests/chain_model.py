"""The whole chain around the effect chain, composed from the stage models in the order pythoncrt_amd/ends.py states, and the seeded
draw of admitted option sets the sweep tests run (tests/test_chain_sweep.py, tests/test_chain_sweep_gpu.py).  No torch and no device here.

A case is a dict: "id", "render" (h, w), "sizes" (the source size of every source frame, in stream order), "batch" (the requested one),
"seed" (of the source frames), "in_cube" / "deliver_cube" ((N, seed) of a lut3d_model.random_table, or None) and "kw", every option
keyword of `process_frames` but the two cubes.  `keywords(case)` is what `process_frames` takes, `raw(case)` what `options.refuse` takes.

`source_stages(case, hw)` / `delivery_stages(case)` are the wiring the models state — which stage stands where, the size and sample type of
what it writes, and how many frames it writes per source frame or per frame of the chain — without a byte computed; `batches(case)` restates
the render loop's batches.  `expect(case, chain)` walks frames through them:
it returns the frames the writer gets and the trace, per batch of the render loop the list of (stage name, frame size, dtype name, frames)
behind every stage, "chain" among them.  `chain(frames, lengths)` is the effect chain over all frames the source ends wrote, `lengths`
the number of them in every batch (`batches(case)` holds the SOURCE frames of every batch; a batch runs `ratio` frames for each)."""
import functools

import numpy as np

from pythoncrt_amd import field420, formats, options, sited, tables
from pythoncrt_amd.depth import DITHERS
from tests import (adeint_model, canvas_model, deep444_model, deep_model, deint_model, depth_model, egress_sited_model, field420_model,
                   interlace_model, lut3d_model, pil_resize_model, resample_model, resize16_model, signal_model, sited_model, unpack_model,
                   yuv422_model, yuv_model)

N_DRAWS = 48
RENDERS = ((24, 40), (23, 37), (16, 24), (18, 56))
SRC_ABOVE = ((48, 72), (31, 57), (36, 64), (30, 44))
SRC_BELOW = ((12, 20), (17, 29), (14, 22))
DELIVER_ABOVE = ((36, 64), (48, 72), (40, 44), (27, 80))
DELIVER_BELOW = ((12, 16), (15, 31), (10, 22), (14, 12))
MATRICES, RANGES = ("bt601", "bt709"), ("tv", "pc")
CUBE_SIZES = (17, 33)
METHODS = deint_model.METHODS + ("adaptive",)
KINDS = ("sited source", "field-paired source", "Signal", "Deinterlace", "AdaptiveDeinterlace", "source crop", "source resize", "Widen",
         "in_lut", "deliver_lut", "delivery resize", "pad Canvas", "crop Canvas", "Interlace", "Narrow", "sited egress")
# the pairs of kinds that cannot stand in one chain: one source plan, one deinterlacer and one delivery Canvas are built
EXCLUSIVE = (("sited source", "field-paired source"), ("Deinterlace", "AdaptiveDeinterlace"), ("pad Canvas", "crop Canvas"))
DEFAULTS = dict(in_pix_fmt="rgb24", in_matrix="bt601", in_range="tv", in_size=None, in_chroma="replicate", in_chroma_rows="progressive",
                in_filter="bilinear", in_crop=None, in_signal="rgb", signal_chroma="sharp", signal_crawl=True, deinterlace="off", field_order="tff",
                deinterlace_fields="first", chain_pix="auto", dither="none", out_pix_fmt="rgb24", out_matrix="bt601", out_range="tv",
                out_chroma="center", deliver_size=None, deliver_filter="bilinear", deliver_fit="stretch", deliver_pad_color=(0, 0, 0),
                deliver_interlace="off", deliver_lowpass="none")


def _case(name, render, sizes, batch, seed=0, in_cube=None, deliver_cube=None, **kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return {"id": name, "render": tuple(render), "sizes": [tuple(s) for s in sizes], "batch": int(batch), "seed": int(seed), "in_cube": in_cube,
            "deliver_cube": deliver_cube, "kw": {**DEFAULTS, **kw}}


# ---- the draw ---------------------------------------------------------------------------------------------------------------------------------------

def draw(seed):
    """One admitted case, built option by option so that every rule of options.RULES / FIELD_RULES holds by construction: nothing is drawn
    and discarded."""
    rng = np.random.default_rng([int(seed), 0xC4A1])

    def pick(seq):
        return seq[int(rng.integers(len(seq)))]

    def flip(p=0.5):
        return bool(rng.random() < p)
    F = formats.PIX_FMTS
    kw = dict(in_pix_fmt=F[seed % len(F)], out_pix_fmt=F[(3 * seed + seed // len(F)) % len(F)])
    fmt, out = kw["in_pix_fmt"], kw["out_pix_fmt"]
    deep_in, deep_out = formats.bits(fmt) == 10, formats.bits(out) == 10
    kw["chain_pix"] = "half" if deep_in != deep_out or flip(0.3) else "auto"              # one 10-bit end: only under "half"
    if kw["chain_pix"] == "half" and not deep_out:
        kw["dither"] = pick(DITHERS)
    # the source plan
    if fmt in field420.LAYOUTS and flip(0.6):
        kw["in_chroma_rows"] = "interlaced"
    paired = kw.get("in_chroma_rows") == "interlaced"
    if fmt in sited.LAYOUTS:
        kw["in_chroma"] = pick(("replicate", "left", "center"))
    kw["in_matrix"], kw["in_range"], kw["out_matrix"], kw["out_range"] = pick(MATRICES), pick(RANGES), pick(MATRICES), pick(RANGES)
    render = pick([r for r in RENDERS if r[0] % 2 == 0] if paired else RENDERS)          # field-paired rows: an even source height of at least 4
    # the source size and the window
    crop_on = flip(0.45)
    if deep_in:                                                                            # no resize: the source, or its window, has the render size
        src = (render[0] + 6, render[1] + 8) if crop_on else render
        if crop_on:
            kw["in_crop"] = (pick((1, 3, 5)), pick((1, 3, 5, 7))) + render
    else:
        mode = pick(("same", "above", "above", "below"))
        even = (lambda s: [x for x in s if x[0] % 2 == 0]) if paired else list
        src = render if mode == "same" else pick(even(SRC_ABOVE if mode == "above" else SRC_BELOW))
    n = pick((5, 6, 7))
    sizes = [src] * n
    if fmt == "rgb24" and flip(0.5):                                                       # rgb24 frames bring their size: a second one, from frame k on
        other = pick([s for s in SRC_ABOVE + RENDERS[:1] + (render,) if s != src])
        k = int(rng.integers(1, n))
        sizes = [src] * k + [other] * (n - k)
    if crop_on and not deep_in:
        sh, sw = min(s[0] for s in sizes), min(s[1] for s in sizes)
        y, x = pick((1, 3)), pick((1, 3))
        if flip(0.3) and sh >= render[0] + y and sw >= render[1] + x:
            kw["in_crop"] = (y, x) + render                                                # a window of the render size: no resize behind it
        else:
            kw["in_crop"] = (y, x, sh - y - pick((0, 1, 2)), sw - x - pick((0, 1, 3)))
    if fmt != "rgb24" and src != render:
        kw["in_size"] = src
    kw["in_filter"] = pick(tables.RESAMPLE_FILTERS)
    if flip(0.5):
        kw["in_signal"], kw["signal_chroma"], kw["signal_crawl"] = pick(signal_model.SIGNALS), pick(signal_model.CHROMAS), flip()
    if flip(0.6):
        kw["deinterlace"], kw["field_order"], kw["deinterlace_fields"] = pick(METHODS), pick(deint_model.ORDERS), pick(deint_model.FIELDS)
    in_cube = (pick(CUBE_SIZES), 100 + seed) if flip(0.45) else None
    # the delivery
    deliver_cube = (pick(CUBE_SIZES), 200 + seed) if flip(0.45) else None
    if flip(0.65):
        kw["deliver_size"] = pick([d for d in (DELIVER_ABOVE if flip() else DELIVER_BELOW) if d != render])
        kw["deliver_filter"], kw["deliver_fit"] = pick(tables.RESAMPLE_FILTERS), pick(("stretch", "pad", "crop"))
        if kw["deliver_fit"] == "pad":
            kw["deliver_pad_color"] = (7 + seed, 200, 33)
    if flip(0.5):
        kw["deliver_interlace"], kw["deliver_lowpass"] = pick(interlace_model.ORDERS), pick(interlace_model.LOWPASS)
    if out in sited.LAYOUTS and flip(0.6):
        kw["out_chroma"] = "left"
    return _case(f"draw{seed:02d}", render, sizes, pick((2, 3, 4)), seed, in_cube, deliver_cube, **kw)


def draws():
    return [draw(seed) for seed in range(N_DRAWS)]


_FULL = dict(in_signal="composite", in_filter="bicubic", chain_pix="half", deliver_filter="lanczos", deliver_pad_color=(9, 180, 77))

# What the seeds do not reach, and the ends with every stage present.  Over {sited, field-paired} x {Deinterlace, Adaptive} x {pad, crop}
# the four full houses hold every pair; each has all 14 stages of the issue's list.
EXPLICIT = (
    _case("full-sited-deint-pad", (24, 40), [(36, 64)] * 5, 3, 1, (17, 301), (33, 302), in_pix_fmt="yuv422p", in_size=(36, 64), in_chroma="left",
          in_crop=(1, 3, 33, 58), deinterlace="edge", deinterlace_fields="both", out_pix_fmt="nv12", out_chroma="left", deliver_size=(36, 64),
          deliver_fit="pad", deliver_interlace="tff", deliver_lowpass="linear", dither="ordered", **_FULL),
    _case("full-sited-adaptive-crop", (23, 37), [(31, 57)] * 6, 3, 2, (33, 303), (17, 304), in_pix_fmt="nv12", in_size=(31, 57), in_chroma="center",
          in_crop=(3, 1, 27, 55), deinterlace="adaptive", field_order="bff", deinterlace_fields="both", out_pix_fmt="uyvy422", out_chroma="left",
          deliver_size=(15, 31), deliver_fit="crop", deliver_interlace="bff", deliver_lowpass="complex", dither="ordered", **_FULL),
    _case("full-paired-deint-crop", (16, 24), [(30, 44)] * 5, 2, 3, (17, 305), (17, 306), in_pix_fmt="yuv420p", in_size=(30, 44), in_chroma="left",
          in_chroma_rows="interlaced", in_crop=(1, 1, 28, 41), deinterlace="linear", field_order="bff", out_pix_fmt="yuv420p", out_chroma="left",
          deliver_size=(40, 44), deliver_fit="crop", deliver_interlace="tff", deliver_lowpass="complex", dither="none", **_FULL),
    _case("full-paired-adaptive-pad", (18, 56), [(48, 72)] * 7, 3, 4, (33, 307), (33, 308), in_pix_fmt="nv12", in_size=(48, 72),
          in_chroma_rows="interlaced", in_crop=(3, 3, 44, 66), deinterlace="adaptive", deinterlace_fields="both", out_pix_fmt="yuyv422",
          out_chroma="left", deliver_size=(14, 12), deliver_fit="pad", deliver_interlace="bff", deliver_lowpass="none", dither="ordered", **_FULL),
    # the pairs the issue names as never met
    _case("paired-signal-crop", (24, 40), [(30, 48)] * 5, 2, 5, in_pix_fmt="p010le", out_pix_fmt="gbrp10le", in_size=(30, 48), in_crop=(5, 7, 24, 40),
          in_chroma_rows="interlaced", in_chroma="center", in_signal="svideo", signal_chroma="soft", signal_crawl=False),
    _case("crop-weave-ordered", (24, 40), [(24, 40)] * 5, 3, 6, chain_pix="half", dither="ordered", deliver_size=(40, 44), deliver_fit="crop",
          deliver_interlace="bff", deliver_lowpass="linear"),
    _case("in-lut-widen-bicubic", (23, 37), [(31, 57)] * 5, 2, 7, (33, 309), None, in_pix_fmt="uyvy422", in_size=(31, 57), in_filter="bicubic",
          chain_pix="half", out_pix_fmt="x2rgb10le"),
    # a uint8 chain that doubles its frames and weaves them again, at an odd requested batch
    _case("u8-both-weave-batch3", (16, 24), [(16, 24)] * 5, 3, 8, in_pix_fmt="yuyv422", out_pix_fmt="yuv422p", deinterlace="linear",
          deinterlace_fields="both", deliver_interlace="tff"),
    _case("u8-first-weave-batch3", (23, 37), [(23, 37)] * 7, 3, 9, deinterlace="edge", deliver_interlace="bff", deliver_lowpass="complex"),
    _case("half-both-weave-batch3", (24, 40), [(24, 40)] * 5, 3, 10, in_pix_fmt="yuv444p10le", out_pix_fmt="yuv420p10le", out_chroma="left",
          deinterlace="adaptive", deinterlace_fields="both", deliver_interlace="bff", deliver_lowpass="linear"),
    # rgb24 frames uploaded straight into the chain's input between batches that go through a source end of another size
    _case("rgb24-direct-and-off-size", (23, 37), [(23, 37), (23, 37), (31, 57), (31, 57), (31, 57), (23, 37), (23, 37)], 2, 12, in_filter="lanczos",
          out_pix_fmt="yuv420p", out_matrix="bt709"),
    _case("half-both-plain-batch3",(24, 40), [(24, 40)] * 5, 3, 11, in_pix_fmt="x2rgb10le", out_pix_fmt="p010le", deinterlace="edge",
          field_order="bff", deinterlace_fields="both"),
)


def cases():
    return draws() + list(EXPLICIT)


# ---- what a case means --------------------------------------------------------------------------------------------------------------------------

def cube_table(spec):
    return None if spec is None else lut3d_model.random_table(*spec)


def cube(spec):
    """The Cube whose quantised table is `cube_table(spec)`."""
    from pythoncrt_amd.cube import Cube
    if spec is None:
        return None
    t = cube_table(spec)
    c = Cube(spec[0], t.astype(np.float64) / 1020.0)
    assert np.array_equal(c.quantise(), t)
    return c


def keywords(case):
    """The option keywords of process_frames for the case (not batch, noise_seed or the frames)."""
    return {**case["kw"], "in_lut": cube(case["in_cube"]), "deliver_lut": cube(case["deliver_cube"])}


def raw(case):
    return options.Raw(render_hw=case["render"], resize_on="device", **keywords(case))


class Derived:
    """What ends.depth_stages, ChainOptions.ratio / batch / direct state, restated."""

    def __init__(self, case):
        kw = case["kw"]
        self.deep_in, self.deep_out = kw["in_pix_fmt"] in deep_model.LAYOUTS + deep444_model.FORMATS, kw["out_pix_fmt"] in deep_model.LAYOUTS + deep444_model.FORMATS
        forced = kw["chain_pix"] == "half"
        self.half = forced or (self.deep_in and self.deep_out)
        self.widen = forced and not self.deep_in
        self.narrow = kw["dither"] if forced and not self.deep_out else None
        self.ratio = 2 if kw["deinterlace"] != "off" and kw["deinterlace_fields"] == "both" else 1
        self.weave = kw["deliver_interlace"] != "off"
        self.pix = "float16" if self.half else "uint8"
        self.src_dtype = "float16" if self.deep_in else "uint8"                # the stages in front of a Widen run on uint8
        B = max(1, case["batch"])
        if self.ratio == 2 or self.weave:                                     # the chain's frames come or go in pairs
            B = max(2, B - B % 2)
        self.B, self.Bs = B, B // self.ratio
        self.direct = (kw["in_pix_fmt"] == "rgb24" and kw["in_crop"] is None and not self.widen and kw["deinterlace"] == "off" and case["in_cube"] is None
                       and kw["in_signal"] == "rgb")

    def delivered(self, m):
        return -(-m // 2) if self.weave else m


def batches(case):
    """(first source frame, source frames, source size) of every batch as the render loop forms them: at most Bs frames, cut where the size changes."""
    d, out, i, sizes = Derived(case), [], 0, case["sizes"]
    while i < len(sizes):
        n = 1
        while n < d.Bs and i + n < len(sizes) and sizes[i + n] == sizes[i]:
            n += 1
        out.append((i, n, sizes[i]))
        i += n
    return out


def family_of(fmt):
    """The name of a packed format's family of stages."""
    return {formats.YUV420: "yuv420", formats.YUV422: "yuv422", formats.DEEP420: "deep420", formats.DEEP444: "deep444"}[formats.FORMATS[fmt]]


def source_family(case):
    kw = case["kw"]
    fmt = kw["in_pix_fmt"]
    if fmt == "rgb24":
        return None
    if kw["in_chroma_rows"] == "interlaced":
        return "field420"
    if kw["in_chroma"] != "replicate":
        return "sited"
    return family_of(fmt)


def egress_family(case):
    kw = case["kw"]
    fmt = kw["out_pix_fmt"]
    if fmt == "rgb24":
        return None
    if kw["out_chroma"] != "center":
        return "sited"
    return family_of(fmt)


def source_stages(case, hw):
    """[(name, size, dtype name, frames written per source frame)] of the source end of frames of `hw`; [] where frames are uploaded straight
    into the chain's input."""
    kw, d, render = case["kw"], Derived(case), case["render"]
    out, per, cut = [], 1, tuple(hw)
    fam = source_family(case)
    if fam is not None:
        out.append(("source:" + fam, cut, d.src_dtype, 1))
    if kw["in_signal"] != "rgb":
        out.append(("signal", cut, d.src_dtype, 1))
    if kw["deinterlace"] != "off":
        per = d.ratio
        out.append(("adaptive" if kw["deinterlace"] == "adaptive" else "deinterlace", cut, d.src_dtype, per))
    if kw["in_crop"] is not None:
        cut = tuple(kw["in_crop"][2:])
        out.append(("crop", cut, d.src_dtype, per))
    if cut != render:
        out.append(("resize", render, d.src_dtype, per))
    if d.widen:
        out.append(("widen", render, "float16", per))
    if case["in_cube"] is not None:
        out.append(("in_lut", render, d.pix, per))
    return out


def delivery_geometry(case):
    """(inner, at, window, size) of the delivery, as DeliveryEnd derives them."""
    kw, render = case["kw"], case["render"]
    deliver = kw["deliver_size"] if kw["deliver_size"] is not None and tuple(kw["deliver_size"]) != render else None
    size = tuple(deliver) if deliver is not None else render
    inner, at = canvas_model.fit_pad(render, size) if deliver is not None and kw["deliver_fit"] == "pad" else (size, (0, 0))
    window = canvas_model.fit_crop(render, size) if deliver is not None and kw["deliver_fit"] == "crop" else (0, 0) + render
    return deliver, tuple(inner), tuple(at), tuple(window), size


def delivery_stages(case):
    """[(name, size, dtype name, halves the frames?)] of the delivery end, the egress plan last where there is one."""
    d, render = Derived(case), case["render"]
    deliver, inner, at, window, size = delivery_geometry(case)
    out = []
    if case["deliver_cube"] is not None:
        out.append(("deliver_lut", render, d.pix))
    if inner != size:
        if inner != render:
            out.append(("deliver_resize", inner, d.pix))
        out.append(("pad", size, d.pix))
    elif window[2:] != render:
        out.append(("crop_canvas", window[2:], d.pix))
        if window[2:] != size:
            out.append(("deliver_resize", size, d.pix))
    elif deliver is not None:
        out.append(("deliver_resize", size, d.pix))
    if d.weave:
        out.append(("interlace", size, d.pix))
    if d.narrow is not None:
        out.append(("narrow", size, "uint8"))
    fam = egress_family(case)
    if fam is not None:
        out.append(("egress:" + fam, size, "uint8"))
    woven, res = False, []
    for name, hw, dt in out:
        woven = woven or name == "interlace"
        res.append((name, hw, dt, woven))
    return res


KIND_OF = {"source:sited": "sited source", "source:field420": "field-paired source", "signal": "Signal", "deinterlace": "Deinterlace",
           "adaptive": "AdaptiveDeinterlace", "crop": "source crop", "resize": "source resize", "widen": "Widen", "in_lut": "in_lut",
           "deliver_lut": "deliver_lut", "deliver_resize": "delivery resize", "pad": "pad Canvas", "crop_canvas": "crop Canvas",
           "interlace": "Interlace", "narrow": "Narrow", "egress:sited": "sited egress"}


def kinds(case):
    """The stage kinds of KINDS the case builds, over all its source sizes."""
    names = {s[0] for hw in set(case["sizes"]) for s in source_stages(case, hw)} | {s[0] for s in delivery_stages(case)}
    return {KIND_OF[n] for n in names if n in KIND_OF}


def delivered_count(case):
    d = Derived(case)
    return sum(d.delivered(n * d.ratio) for _, n, _ in batches(case))


# ---- the frames -------------------------------------------------------------------------------------------------------------------------------------

def frames(case):
    """The source frames as process_frames takes them, made as tests/test_adeint_pipeline_gpu._frames makes them: one sequence per source
    size, part of the picture standing still from frame to frame."""
    from tests.test_adeint_pipeline_gpu import _frames
    fmt, order = case["kw"]["in_pix_fmt"], []
    for s in case["sizes"]:
        if s not in order:
            order.append(s)
    made = {s: iter(_frames(fmt, s, seed=case["seed"] + 17 * k, n=case["sizes"].count(s))) for k, s in enumerate(order)}
    return [next(made[s]) for s in case["sizes"]]


def unpack_source(case, items, hw):
    """The source model of the format's family over a batch of packed frames: [n, h, w, 3]."""
    kw, fam = case["kw"], source_family(case)
    fmt, m, r, (h, w) = kw["in_pix_fmt"], kw["in_matrix"], kw["in_range"], hw
    one = {"field420": lambda p: field420_model.unpack(p, h, w, fmt, kw["in_chroma"], m, r),
           "sited": lambda p: sited_model.unpack(p, h, w, fmt, kw["in_chroma"], m, r),
           "yuv420": lambda p: unpack_model.unpack(p, h, w, fmt, m, r), "yuv422": lambda p: yuv422_model.unpack(p, h, w, fmt, m, r),
           "deep420": lambda p: deep_model.unpack(p, h, w, fmt, m, r), "deep444": lambda p: deep444_model.unpack(p, h, w, fmt, m, r)}[fam]
    return np.stack([one(np.asarray(p).reshape(-1)) for p in items])


def pack_egress(case, rgb):
    """The egress model of the family and siting over a batch: [n, frame_bytes] uint8."""
    kw, fam = case["kw"], egress_family(case)
    fmt, m, r = kw["out_pix_fmt"], kw["out_matrix"], kw["out_range"]
    one = {"sited": lambda f: egress_sited_model.pack(f, fmt, kw["out_chroma"], m, r), "yuv420": lambda f: yuv_model.pack(f, fmt, m, r),
           "yuv422": lambda f: yuv422_model.pack(f, fmt, m, r), "deep420": lambda f: deep_model.pack(f, fmt, m, r),
           "deep444": lambda f: deep444_model.pack(f, fmt, m, r)}[fam]
    return np.stack([one(f) for f in rgb])


def resize(x, hw, filter):     # noqa: A002 - the stages' keyword
    """The resize model of the sample type and filter over a batch."""
    if x.dtype == np.uint8:
        one = (lambda f: pil_resize_model.resize(f, *hw)) if filter == "bilinear" else (lambda f: resample_model.resize_u8(f, hw[0], hw[1], filter))
        return np.stack([one(f) for f in x])
    assert x.dtype == np.float16
    return resize16_model.resize(x, *hw) if filter == "bilinear" else resample_model.resize_half(x, hw[0], hw[1], filter)


def source_side(case):
    """The source ends over the stream: per batch the list of (name, size, dtype name, frames) behind every stage.  A batch uploaded
    straight into the chain has the one entry "upload"."""
    kw, d, out = case["kw"], Derived(case), []
    items, prev, last_hw = frames(case), None, None
    in_table = cube_table(case["in_cube"])
    for lo, n, hw in batches(case):
        plan = source_stages(case, hw)
        x = np.stack(items[lo:lo + n]) if kw["in_pix_fmt"] == "rgb24" else None
        if hw != last_hw:
            prev = None                                                      # a new history starts where the source size changes
        last_hw, trace = hw, []
        for name, size, dt, per in plan:
            if name.startswith("source:"):
                x = unpack_source(case, items[lo:lo + n], hw)
            elif name == "signal":
                x = signal_model.signal(x, kw["in_signal"], kw["signal_chroma"], kw["signal_crawl"], index=lo)
            elif name == "deinterlace":
                x = deint_model.deinterlace(x, kw["deinterlace"], kw["field_order"], kw["deinterlace_fields"])
            elif name == "adaptive":
                x, prev = adeint_model.adaptive(x, prev, kw["field_order"], kw["deinterlace_fields"]), x[-1]
            elif name == "crop":
                x = canvas_model.crop(x, tuple(kw["in_crop"]))
            elif name == "resize":
                x = resize(x, size, kw["in_filter"])
            elif name == "widen":
                x = depth_model.widen(x)
            elif name == "in_lut":
                x = lut3d_model.apply(x, in_table)
            assert x.shape == (n * per,) + size + (3,) and x.dtype == np.dtype(dt), (case["id"], name, x.shape, x.dtype, size, dt)
            trace.append((name, size, dt, x))
        if not plan:
            assert d.direct and hw == case["render"] and x.dtype == np.uint8
            trace.append(("upload", hw, "uint8", x))
        out.append(trace)
    return out


def delivery_side(case, chain_out, lengths):
    """The delivery end over the chain's frames, batch by batch: per batch the list of (name, size, dtype name, frames) behind every stage."""
    kw, out, lo = case["kw"], [], 0
    deliver, inner, at, window, size = delivery_geometry(case)
    table = cube_table(case["deliver_cube"])
    for m in lengths:
        x, trace = chain_out[lo:lo + m], []
        lo += m
        for name, hw, dt, woven in delivery_stages(case):
            if name == "deliver_lut":
                x = lut3d_model.apply(x, table)
            elif name == "deliver_resize":
                x = resize(x, hw, kw["deliver_filter"])
            elif name == "pad":
                x = canvas_model.canvas(x, size, at=at, fill=np.array(kw["deliver_pad_color"], dtype=x.dtype))
            elif name == "crop_canvas":
                x = canvas_model.crop(x, window)
            elif name == "interlace":
                x = interlace_model.interlace(x, kw["deliver_interlace"], kw["deliver_lowpass"])       # an odd last frame is woven with itself
            elif name == "narrow":
                x = depth_model.narrow(x, kw["dither"])
            elif name.startswith("egress:"):
                x = pack_egress(case, x)
                assert x.shape == (-(-m // 2) if woven else m, formats.frame_bytes(hw[0], hw[1], kw["out_pix_fmt"])) and x.dtype == np.uint8
                trace.append((name, hw, dt, x))
                continue
            assert x.shape == ((-(-m // 2) if woven else m),) + hw + (3,) and x.dtype == np.dtype(dt), (case["id"], name, x.shape, x.dtype, hw, dt)
            trace.append((name, hw, dt, x))
        out.append((x, trace))
    return out


def identity(x, lengths):
    return x


def expect(case, chain=identity, source=None):
    """(the frames the writer gets, the trace).  `source`: a source_side(case) computed earlier (it does not depend on the chain)."""
    d = Derived(case)
    source = source_side(case) if source is None else source
    lengths = [n * d.ratio for _, n, _ in batches(case)]
    chain_in = np.concatenate([t[-1][3] for t in source])
    assert chain_in.shape == (sum(lengths),) + case["render"] + (3,) and chain_in.dtype == np.dtype(d.pix), (case["id"], chain_in.shape, chain_in.dtype)
    chain_out = np.asarray(chain(chain_in, lengths))
    assert chain_out.shape == chain_in.shape and chain_out.dtype == chain_in.dtype
    sent, trace, lo = [], [], 0
    for src, m, (x, behind) in zip(source, lengths, delivery_side(case, chain_out, lengths)):
        trace.append(list(src) + [("chain", case["render"], d.pix, chain_out[lo:lo + m])] + behind)
        lo += m
        sent.extend(x)
    assert len(sent) == delivered_count(case)
    return sent, trace


@functools.lru_cache(maxsize=None)
def _cached_source(case_id):
    return source_side({c["id"]: c for c in cases() + list(STREAMS)}[case_id])


def cached_source(case):
    """source_side(case), computed once for the tests that share it and never written to."""
    return _cached_source(case["id"])


# ---- the explicit streams of the GPU sweep: rgb24, batch 2 ---------------------------------------------------------------------------------------

_A, _B, _C, _D, _E, _F = (24, 40), (30, 44), (31, 57), (36, 64), (17, 29), (48, 72)
_SIX = [_A, _A, _B, _B, _C, _C, _D, _D, _E, _E, _A, _A, _F]           # A's second visit comes after four other sizes: its source end was dropped
STREAMS = (
    _case("six-sizes", _A, _SIX, 2, 21, in_signal="composite", deinterlace="adaptive", deinterlace_fields="both", in_filter="bicubic"),
    _case("six-sizes-crop-half", (16, 24), _SIX, 2, 22, in_signal="composite", deinterlace="adaptive", deinterlace_fields="both", in_filter="bicubic",
          in_crop=(1, 3, 15, 23), chain_pix="half"),
    _case("odd-run-weave-pad", _A, [_A, _A, _A, _B, _B, _A, _A], 2, 23, chain_pix="half", dither="ordered", deliver_interlace="bff",
          deliver_lowpass="complex", deliver_size=(36, 44), deliver_fit="pad", deliver_pad_color=(9, 180, 77)),
)
