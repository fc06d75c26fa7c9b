"""The two callers of the chain ends (pythoncrt_amd/ends.py) held to each other: `cli.main`, file to file, and `process_frames` over the
same frames write the same bytes, for a source and an egress plan of every family, sited chroma on either end, and a delivery resize under
three filters.  7 frames in batches of 3 — the last batch is partial, and the default persistence of 0.2 carries state across batches.
Exact: there is no tolerance.  Then the aliasing rule of DeliveryEnd.slots on its own."""
import numpy as np
import pytest

from pythoncrt_amd import formats

pytestmark = pytest.mark.gpu

N, BATCH, SEED = 7, 3, 19
SIZES = [(72, 128), (37, 66)]               # every format takes odd sizes (chroma planes round up)
# in_pix_fmt, in_chroma, out_pix_fmt, out_chroma, delivery size, its filter
CASES = [("rgb24", "replicate", "rgb24", "center", None, "bilinear"),
         ("nv12", "replicate", "yuv420p", "center", None, "bilinear"),
         ("yuv420p", "left", "nv12", "left", None, "bilinear"),
         ("uyvy422", "replicate", "yuv422p", "left", None, "bilinear"),
         ("p010le", "replicate", "yuv420p10le", "center", None, "bilinear"),
         ("yuv444p10le", "replicate", "x2rgb10le", "center", None, "bilinear"),
         ("gbrp10le", "replicate", "p010le", "left", None, "bilinear"),
         ("rgb24", "replicate", "yuv420p", "center", (36, 64), "bilinear"),
         ("rgb24", "replicate", "rgb24", "center", (36, 64), "lanczos"),
         ("p010le", "replicate", "p010le", "center", (36, 64), "bicubic")]


def _frames(fmt, size):
    """N frames of `fmt` as process_frames takes them: H x W x 3 for rgb24, else 1-D uint8 of frame_bytes; 10-bit samples are valid ones."""
    h, w = size
    rng = np.random.default_rng([h, w, len(fmt), sum(map(ord, fmt))])
    nb = formats.frame_bytes(h, w, fmt)
    if fmt == "rgb24":
        return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(N)]
    if formats.bits(fmt) == 8:
        return [rng.integers(0, 256, nb, dtype=np.uint8) for _ in range(N)]
    if fmt == "x2rgb10le":
        return [rng.integers(0, 1 << 30, nb // 4, dtype=np.uint32).astype("<u4").view(np.uint8) for _ in range(N)]
    shift = 6 if fmt == "p010le" else 0
    return [(rng.integers(0, 1024, nb // 2, dtype=np.uint16) << shift).astype("<u2").view(np.uint8) for _ in range(N)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{'x'.join(map(str, c[4])) + c[5] if c[4] else 'asrendered'}")
def test_cli_and_process_frames_write_the_same_bytes(tmp_path, case, size):
    import pythoncrt_amd as pc
    from pythoncrt_amd import cli
    in_fmt, in_chroma, out_fmt, out_chroma, deliver, flt = case
    h, w = size
    items = _frames(in_fmt, size)
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    src.write_bytes(b"".join(a.tobytes() for a in items))
    flags = ["--input", str(src), "--output", str(dst), "--width", str(w), "--height", str(h), "--fps", "30", "--batch", str(BATCH),
             "--noise-seed", str(SEED), "--in-pix-fmt", in_fmt, "--in-chroma", in_chroma, "--out-pix-fmt", out_fmt, "--out-chroma", out_chroma]
    kw = dict(in_pix_fmt=in_fmt, in_chroma=in_chroma, out_pix_fmt=out_fmt, out_chroma=out_chroma)
    if deliver is not None:
        flags += ["--deliver-height", str(deliver[0]), "--deliver-width", str(deliver[1]), "--deliver-filter", flt]
        kw.update(deliver_size=deliver, deliver_filter=flt)
    assert cli.main(flags) == 0
    got = []
    wrote = pc.process_frames(iter(items), lambda a: got.append(np.array(a).reshape(-1)), w, h, 30, N, noise_seed=SEED, batch=BATCH, **kw)
    dh, dw = deliver or size
    fb = formats.frame_bytes(dh, dw, out_fmt)
    assert wrote == N == len(got) and all(a.dtype == np.uint8 and a.size == fb for a in got)
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[N - 2], got[N - 1])      # frames of a render, not one constant
    written = np.frombuffer(dst.read_bytes(), dtype=np.uint8)
    assert written.size == N * fb, (written.size, N, fb)
    bad = [i for i in range(N) if not np.array_equal(written[i * fb:(i + 1) * fb], got[i])]
    assert not bad, (case, size, bad)


def test_delivery_end_slots_alias_where_a_stage_is_missing():
    """DeliveryEnd.slots at 8 x 16: a missing stage costs no buffer — without a resize fin is dev_out, without an egress plan send is fin."""
    import torch
    from pythoncrt_amd.ends import DeliveryEnd
    dev = torch.device("cuda", torch.cuda.current_device())
    dev_out = [torch.empty((2, 8, 16, 3), dtype=torch.uint8, device=dev) for _ in range(3)]

    def ptrs(ts):
        return [t.data_ptr() for t in ts]
    fin, send = DeliveryEnd(dev, (8, 16), torch.uint8, "rgb24", "bt601", "tv", "center", None, "bilinear").slots(dev_out)
    assert ptrs(fin) == ptrs(send) == ptrs(dev_out) and all(a is b is c for a, b, c in zip(fin, send, dev_out))
    end = DeliveryEnd(dev, (8, 16), torch.uint8, "nv12", "bt601", "tv", "center", None, "bilinear")
    fin, send = end.slots(dev_out)
    assert all(a is b for a, b in zip(fin, dev_out)) and not set(ptrs(send)) & set(ptrs(dev_out)) and len(set(ptrs(send))) == 3
    assert all(tuple(t.shape) == (2, formats.frame_bytes(8, 16, "nv12")) == end.shape(2) and t.dtype == torch.uint8 for t in send)
    end = DeliveryEnd(dev, (8, 16), torch.uint8, "nv12", "bt601", "tv", "center", (4, 8), "bilinear")
    fin, send = end.slots(dev_out)
    assert len(set(ptrs(fin)) | set(ptrs(send)) | set(ptrs(dev_out))) == 9
    assert all(tuple(t.shape) == (2, 4, 8, 3) for t in fin) and all(tuple(t.shape) == (2, formats.frame_bytes(4, 8, "nv12")) for t in send)
    fin, send = DeliveryEnd(dev, (8, 16), torch.uint8, "rgb24", "bt601", "tv", "center", (4, 8), "bilinear").slots(dev_out)      # a resize only
    assert all(a is b for a, b in zip(fin, send)) and not set(ptrs(fin)) & set(ptrs(dev_out))
