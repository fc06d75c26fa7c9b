"""Which plan stands at each end of the chain (formats.source_plan / formats.egress_plan) and what ends.DeliveryEnd hands downstream, against
tables written out here.  The plan classes' constructors are replaced by recorders: no GPU."""
import pytest
import torch

from pythoncrt_amd import _stage, deep, deep444, egress, ends, formats, ingest, resample, resize16, sited, unpack, yuv422

K3, K4 = ("layout", "matrix", "range"), ("layout", "matrix", "range", "siting")
YUV420, YUV422, DEEP420, DEEP444 = ("yuv420p", "nv12"), ("yuv422p", "yuyv422", "uyvy422"), ("yuv420p10le", "p010le"), ("yuv444p10le", "gbrp10le", "x2rgb10le")
# (format, chroma, the class constructed or None, its keywords); what the callers refuse — a siting with rgb24 or a 4:4:4 format — is no row
SOURCES = ([("rgb24", "replicate", None, ())]
           + [(f, "replicate", unpack.UnpackYuv, K3) for f in YUV420] + [(f, "replicate", yuv422.UnpackYuv422, K3) for f in YUV422]
           + [(f, "replicate", deep.UnpackYuv10, K3) for f in DEEP420] + [(f, "replicate", deep444.UnpackDeep444, K3) for f in DEEP444]
           + [(f, c, sited.UnpackSited, K4) for f in YUV420 + YUV422 + DEEP420 for c in ("left", "center")])
EGRESSES = ([("rgb24", "center", None, ())]
            + [(f, "center", egress.EgressYuv, K3) for f in YUV420] + [(f, "center", yuv422.EgressYuv422, K3) for f in YUV422]
            + [(f, "center", deep.EgressYuv10, K3) for f in DEEP420] + [(f, "center", deep444.EgressDeep444, K3) for f in DEEP444]
            + [(f, "left", sited.EgressSited, K4) for f in YUV420 + YUV422 + DEEP420])
STAGES = sorted({row[2] for row in SOURCES + EGRESSES if row[2] is not None}, key=lambda c: c.__name__)
RESIZES = (ingest.IngestResize, resize16.ResizeHalf, resample.Resample)


class Untouchable:
    """A device argument that fails the test when anything is asked of it."""
    def __getattribute__(self, name):
        raise AssertionError(f"the device argument was touched: .{name}")


@pytest.fixture
def built(monkeypatch):
    """Every plan class records (class, positional arguments, keywords) instead of creating its plan; a stage plan still knows its
    frame_bytes, as StagePlan.__init__ sets it."""
    log = []
    for cls in STAGES + list(RESIZES):
        def init(self, *args, _cls=cls, **kw):
            log.append((_cls, args, kw))
            if issubclass(_cls, _stage.StagePlan):
                self.frame_bytes = _cls._frame_bytes(args[1][0], args[1][1], kw["layout"])
        monkeypatch.setattr(cls, "__init__", init)
    return log


def test_the_tables_cover_every_format(built):
    unsited = ("rgb24",) + DEEP444                 # no sub-sampled chroma: the callers refuse every chroma value but the default
    refused = {(f, c) for f in unsited for c in ("left", "center")}
    assert {r[:2] for r in SOURCES} == {(f, c) for f in formats.PIX_FMTS for c in ("replicate", "left", "center")} - refused and len(SOURCES) == 25
    refused = {(f, "left") for f in unsited}
    assert {r[:2] for r in EGRESSES} == {(f, c) for f in formats.PIX_FMTS for c in ("center", "left")} - refused and len(EGRESSES) == 18


@pytest.mark.parametrize("choose,rows", [("source_plan", SOURCES), ("egress_plan", EGRESSES)])
def test_plan_choice(built, choose, rows):
    for fmt, chroma, cls, keys in rows:
        del built[:]
        if cls is None:
            assert getattr(formats, choose)(Untouchable(), (6, 10), fmt, "bt709", "pc", chroma) is None and built == []
            continue
        plan = getattr(formats, choose)("dev", (6, 10), fmt, "bt709", "pc", chroma)
        want = {"layout": fmt, "matrix": "bt709", "range": "pc", "siting": chroma}
        assert type(plan) is cls and built == [(cls, ("dev", (6, 10)), {k: want[k] for k in keys})], (fmt, chroma, built)


@pytest.mark.parametrize("fmt,pix", [("rgb24", torch.uint8), ("nv12", torch.uint8), ("uyvy422", torch.uint8), ("p010le", torch.float16),
                                     ("x2rgb10le", torch.float16)])
@pytest.mark.parametrize("render,deliver,flt", [((72, 128), None, "bilinear"), ((72, 128), (36, 64), "bilinear"), ((37, 66), (18, 32), "lanczos"),
                                                ((37, 66), None, "bilinear")])
def test_delivery_end_sizes(built, fmt, pix, render, deliver, flt):
    """size, frame_bytes and shape(B) are those of the DELIVERY size; the egress plan is built for it; a resize plan exists only with one."""
    end = ends.DeliveryEnd("dev", render, pix, fmt, "bt601", "tv", "center", deliver, flt)
    dh, dw = deliver or render
    assert end.size == (dh, dw) and end.frame_bytes == formats.frame_bytes(dh, dw, fmt)
    assert end.shape(3) == ((3, dh, dw, 3) if fmt == "rgb24" else (3, formats.frame_bytes(dh, dw, fmt)))
    resizes = [b for b in built if b[0] in RESIZES]
    stages = [b for b in built if b[0] in STAGES]
    assert (end.egress is None) == (fmt == "rgb24") and [s[1] for s in stages] == ([] if fmt == "rgb24" else [("dev", (dh, dw))])
    if deliver is None:
        assert end.resize is None and resizes == []
    elif flt == "bilinear":
        assert resizes == [(resize16.ResizeHalf if pix == torch.float16 else ingest.IngestResize, ("dev", render, deliver), {})]
    else:
        assert resizes == [(resample.Resample, ("dev", render, deliver), {"filter": flt, "dtype": pix})]
    assert type(end.resize) is (resizes[0][0] if resizes else type(None))
