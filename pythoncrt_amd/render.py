"""`process_frames` — the hot loop of the reference's `process_video` (crt_filter.py ref:1037-1131) behind a callable a maintainer can drop
into `process_video` itself: the frame iterator the reference already has (`clip.iter_frames(...)` ref:1036 or `FFmpegRawReader.iter_frames()`
ref:1034), the writer call it already makes (`writer.write_frame`, ref:1101) and the effect keywords `process_video` was called with
(ref:864-911, same names).  In `process_video` the lines ref:1015-1131 — thread pool, futures dictionary, in-order drain, persistence blend,
`convertScaleAbs` — become

    n = pythoncrt_amd.process_frames(frame_iter, writer.write_frame, out_w, out_h, fps_out, total_frames,
                                     scanline_strength=scanline_strength, triad_strength=triad_strength, ..., progress_cb=progress_cb)

What it keeps of the reference's loop: frames of another size are resized as Pillow's BILINEAR does first (ref:1039-1041; on the device,
byte for byte Pillow's result — pythoncrt_amd.ingest — or with Pillow itself under `resize_on="host"`); frame i runs at
phase = i / fps * scanline_speed_px_s and time_sec = i / fps (ref:1043, :1064); frames are committed strictly in order, frame 0 passes through
unblended, frame i > 0 blends with the state frame i - 1 left (ref:1086-1096); `progress_cb(min(1, frames_written / total_frames))` after
every frame (ref:1104-1105); the text overlay is rasterised once (ref:1076-1077 builds the same plane for every frame).  What differs: the
frames of a batch go to the GPU together (pinned staging, upload / kernels / download on three streams, batch k's kernels under the host's
writes of batch k - 1 and reads of batch k + 1) instead of one `apply_static_effects` call per frame on two worker threads."""
from __future__ import annotations

import contextlib
from typing import Callable, Iterable, Optional, Tuple

import numpy as np

from . import formats

# process_video keywords that belong to its container / codec plumbing (out of scope): accepted so that a caller can forward its
# own keyword dictionary unchanged, and ignored
_IO_KEYS = ("input_path", "output_path", "width", "height", "fps", "crf", "target_bitrate_kbps", "gpu", "nvenc_preset", "encoder_preference",
            "decoder_preference")


def _iter_frames(stream, frame_size: int):
    """Whole frames of frame_size bytes from an already open byte stream, as 1-D uint8 arrays, until the stream ends; a trailing partial
    frame is dropped."""
    while True:
        buf = stream.read(frame_size)
        while buf and len(buf) < frame_size:           # a pipe may return less than asked for: keep reading until the frame is whole or the stream ends
            more = stream.read(frame_size - len(buf))
            if not more:
                break
            buf += more
        if not buf or len(buf) < frame_size:
            return
        yield np.frombuffer(buf, dtype=np.uint8)


def iter_rgb24(stream, out_w: int, out_h: int):
    """The frame iterator of the reference's FFmpegRawReader.iter_frames (ref:495-506) over an ALREADY OPEN byte stream of raw rgb24 — the
    stdout of an ffmpeg process the caller started (`-f rawvideo -pix_fmt rgb24 -`), a file, a pipe: frames of out_h x out_w x 3 uint8 until the
    stream ends; a trailing partial frame is dropped, as there.  (The reader class itself — spawning ffmpeg, hw-accel flags — is codec plumbing
    and stays the reference's.)"""
    for frame in _iter_frames(stream, formats.frame_bytes(out_h, out_w, "rgb24")):
        yield frame.reshape((int(out_h), int(out_w), 3))


def iter_yuv420(stream, w: int, h: int, bits: int = 8):
    """`iter_rgb24` for an already open byte stream of raw yuv420p or nv12 (`-f rawvideo -pix_fmt yuv420p -` / `-pix_fmt nv12 -`): 1-D uint8
    arrays of frame_bytes = h * w + 2 * ceil(h / 2) * ceil(w / 2) bytes — what `process_frames(..., in_pix_fmt=)` takes — until the stream
    ends; the same short-read handling, a trailing partial frame is dropped.  Both layouts have the same size: the bytes are not interpreted here.
    `bits=10` reads yuv420p10le / p010le (`-pix_fmt yuv420p10le -` / `-pix_fmt p010le -`): the same, with frames of twice as many bytes
    (16-bit little-endian words), still handed out as 1-D uint8 arrays."""
    if bits not in (8, 10):
        raise ValueError(f"bits must be 8 or 10, got {bits!r}")
    return _iter_frames(stream, formats.frame_bytes(h, w, "yuv420p10le" if bits == 10 else "yuv420p"))


def iter_yuv422(stream, w: int, h: int, layout: str):
    """`iter_yuv420` for an already open byte stream of raw yuv422p, yuyv422 or uyvy422 (`-f rawvideo -pix_fmt uyvy422 -`): 1-D uint8 arrays of
    yuv422.frame_bytes(h, w, layout) bytes — what `process_frames(..., in_pix_fmt=layout)` takes — until the stream ends; the same
    short-read handling, a trailing partial frame is dropped.  The bytes are not interpreted here."""
    return _iter_frames(stream, formats.YUV422.frame_bytes(int(h), int(w), layout))


def iter_deep444(stream, w: int, h: int, fmt: str):
    """`iter_yuv422` for an already open byte stream of raw yuv444p10le, gbrp10le or x2rgb10le (`-f rawvideo -pix_fmt gbrp10le -`): 1-D uint8
    arrays of deep444.frame_bytes(h, w, fmt) bytes — what `process_frames(..., in_pix_fmt=fmt)` takes — until the stream ends; the same
    short-read handling, a trailing partial frame is dropped.  The bytes are not interpreted here."""
    return _iter_frames(stream, formats.DEEP444.frame_bytes(int(h), int(w), fmt))


def parse_deliver_size(deliver_size, out_h: int, out_w: int) -> Optional[Tuple[int, int]]:
    """(dh, dw) of `process_frames(deliver_size=)`, or None where the frames are delivered as rendered (None, or the render size itself).
    ValueError: not a pair of integers, a size < 1 or > 32767."""
    if deliver_size is None:
        return None
    try:
        dh, dw = deliver_size
        if isinstance(dh, bool) or isinstance(dw, bool) or int(dh) != dh or int(dw) != dw:
            raise TypeError
        dh, dw = int(dh), int(dw)
    except (TypeError, ValueError):
        raise ValueError(f"deliver_size must be a pair (height, width) of integers, got {deliver_size!r}") from None
    if min(dh, dw) < 1 or max(dh, dw) > 32767:
        raise ValueError(f"deliver_size={deliver_size!r}: sizes outside 1..32767")
    return None if (dh, dw) == (int(out_h), int(out_w)) else (dh, dw)


DELIVER_FITS = ("stretch", "pad", "crop")
CHAIN_PIX = ("auto", "half")        # what the chain runs on: what the formats say (uint8, or half between two 10-bit ends), or half whatever they are


def parse_in_crop(in_crop, bounds: Optional[Tuple[int, int]] = None, name: str = "in_crop") -> Optional[Tuple[int, int, int, int]]:
    """(y, x, h, w) of `process_frames(in_crop=)`, or None.  ValueError: not four integers, a side < 1, an origin < 0, and — where the
    source size `bounds` = (src_h, src_w) is known — a window that leaves it."""
    if in_crop is None:
        return None
    try:
        vals = tuple(in_crop)
        if len(vals) != 4 or any(isinstance(v, bool) or int(v) != v for v in vals):
            raise TypeError
        y, x, ch, cw = (int(v) for v in vals)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be four integers (y, x, height, width), got {in_crop!r}") from None
    if min(ch, cw) < 1 or min(y, x) < 0:
        raise ValueError(f"{name}={(y, x, ch, cw)}: a window needs an origin >= 0 and sides >= 1")
    if bounds is not None and (y + ch > bounds[0] or x + cw > bounds[1]):
        raise ValueError(f"{name}={(y, x, ch, cw)}: the window leaves the {bounds[0]} x {bounds[1]} source frame")
    return y, x, ch, cw


def parse_pad_color(color, name: str = "deliver_pad_color") -> Tuple[int, int, int]:
    """(r, g, b) of `process_frames(deliver_pad_color=)`.  ValueError: not three integers 0..255."""
    try:
        vals = tuple(color)
        if len(vals) != 3 or any(isinstance(v, bool) or int(v) != v for v in vals):
            raise TypeError
        vals = tuple(int(v) for v in vals)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be three integers (r, g, b) in 0..255, got {color!r}") from None
    if min(vals) < 0 or max(vals) > 255:
        raise ValueError(f"{name}={vals}: values outside 0..255")
    return vals


def process_frames(frame_iter: Iterable[np.ndarray], write_frame: Callable[[np.ndarray], None], out_w: int, out_h: int, fps_out: float,
                   total_frames: Optional[int] = None, *,
                   scanline_strength: float = 0.6, triad_strength: float = 0.35, triad_gamma: float = 2.2, triad_preserve_luma: bool = False,
                   triad_softness: float = 0.5, aberration_px: int = 1, bloom_sigma: float = 1.2, bloom_strength: float = 0.25,
                   noise_strength: float = 1.5, vignette_strength: float = 0.25, persistence: float = 0.2, scanline_speed_px_s: float = 30.0,
                   scanline_period_px: float = 2.0, fast_bloom: bool = True, pixel_size: int = 2, glitch_amp_px: int = 0,
                   glitch_height_frac: float = 0.0, bloom_threshold: float = 0.0, brightness: float = 0.0, contrast: float = 1.0,
                   gamma: float = 1.0, saturation: float = 1.0, temperature: float = 0.0, flicker_strength: float = 0.0, flicker_hz: float = 0.0,
                   grain_size: int = 1, scanline_angle: float = 0.0, scanline_thickness: float = 1.0, warp_strength: float = 0.0,
                   text: str = "", text_font: str = "", text_size: int = 36, text_color: str = "#FFFFFF", text_pos: Tuple[int, int] = (32, 32),
                   text_after: bool = True, progress_cb: Optional[Callable[[float], None]] = None,
                   batch: int = 16, noise_seed: Optional[int] = None, device=None, resize_on: str = "device",
                   out_pix_fmt: str = "rgb24", out_matrix: str = "bt601", out_range: str = "tv",
                   in_pix_fmt: str = "rgb24", in_matrix: str = "bt601", in_range: str = "tv", in_size: Optional[Tuple[int, int]] = None,
                   in_chroma: str = "replicate", out_chroma: str = "center", deliver_size: Optional[Tuple[int, int]] = None,
                   in_filter: str = "bilinear", deliver_filter: str = "bilinear", in_crop: Optional[Tuple[int, int, int, int]] = None,
                   deliver_fit: str = "stretch", deliver_pad_color: Tuple[int, int, int] = (0, 0, 0), chain_pix: str = "auto",
                   dither: str = "none", deinterlace: str = "off", field_order: str = "tff", deinterlace_fields: str = "first",
                   in_lut=None, deliver_lut=None, deliver_interlace: str = "off", deliver_lowpass: str = "none",
                   in_signal: str = "rgb", signal_chroma: str = "sharp", signal_crawl: bool = True, in_chroma_rows: str = "progressive",
                   out_chroma_rows: str = "progressive", signal_standard: str = "ntsc", pal_decoder: str = "delay", signal_phase: int = 0,
                   **io_keywords) -> int:
    """Render every frame of `frame_iter` (H x W x 3 uint8 RGB arrays) and hand the finished uint8 frames to `write_frame` in order.
    Effect keywords: the names, meaning and defaults of process_video / the CLI (ref:864-911, :1155-1206); the caller applies the clamps of
    ref:1225-1266 as the reference's `main` does (`pythoncrt_amd.cli.settings_from_args` restates them).  Returns the number of frames written.
    The array passed to `write_frame` is a view of a staging buffer that is reused two batches later: consume it inside the call (the
    reference's `FFMPEG_VideoWriter.write_frame` writes it to the encoder's pipe at once).
    `progress_cb(fraction)` is called after every written frame with min(1, written / total_frames) (ref:1104-1105; the reference always knows
    its total, ref:1029).  With `total_frames=None` no fraction can be formed: the callback is then called ONCE, with 1.0, after the last frame.
    Frames of another size than out_h x out_w are brought to it as `Image.resize((out_w, out_h), Image.BILINEAR)` does (ref:1039-1041):
    with `resize_on="device"` (default) they are uploaded at their own size and resized by the ingest kernels (IngestResize: Pillow's bytes),
    a batch ending early where the source size changes; with `resize_on="host"` by Pillow itself on the calling thread, the reference's
    literal form (kept for A/B).  Both give the same bytes.
    `out_pix_fmt="yuv420p"` / `"nv12"` hands the writer the encoder's format instead of rgb24 (the reference's encoder branches all end in
    `-pix_fmt yuv420p`, ref:970-1002): the finished frames are converted on the device behind the chain (EgressYuv, include/crtfx_egress.h:
    `out_matrix` "bt601" / "bt709", `out_range` "tv" / "pc"), only frame_bytes = h * w + 2 * ceil(h / 2) * ceil(w / 2) bytes per frame are
    downloaded, and `write_frame` receives a 1-D uint8 array of that many bytes.  "rgb24" (default) is the path as it was.
    `in_pix_fmt="yuv420p"` / `"nv12"` takes the decoder's format instead of rgb24: every item of `frame_iter` is then a uint8 array of
    frame_bytes(*in_size) elements (any shape; it is flattened — `iter_yuv420` yields them), `in_size = (src_h, src_w)` defaulting to the
    output size; the frames are staged and uploaded as 1.5 bytes per pixel and converted to RGB on the device in front of the chain
    (UnpackYuv, include/crtfx_unpack.h: `in_matrix` "bt601" / "bt709", `in_range` "tv" / "pc"); where `in_size` differs from the output
    size that RGB is resized by IngestResize.  `resize_on="host"` is refused with it (there is no host RGB frame to hand to Pillow).
    "rgb24" (default) is the path as it was.
    "yuv422p", "yuyv422" and "uyvy422" (8-bit 4:2:2, what capture cards and mezzanine codecs hand out) are members of the same 8-bit family
    on either end, independently of the other end: UnpackYuv422 stands in front of the chain and EgressYuv422 behind it
    (include/crtfx_422.h, the same matrix and range keywords), items of `frame_iter` (`iter_yuv422` yields them) and the arrays handed to
    `write_frame` are 1-D uint8 arrays of yuv422.frame_bytes(h, w, layout) bytes — 2 per pixel — and an off-size 4:2:2 source goes through
    IngestResize behind the source stage as a 4:2:0 one does.
    `in_pix_fmt` and `out_pix_fmt` both "yuv420p10le" / "p010le" (either layout on either end) is the 10-bit path: the chain runs on half
    pixels (FramePipeline(dtype=torch.float16)), UnpackYuv10 stands in front of it and EgressYuv10 behind it (include/crtfx_deep.h, same
    matrix and range keywords), items of `frame_iter` and the arrays handed to `write_frame` are 1-D uint8 arrays of
    2 * (h * w + 2 * ceil(h / 2) * ceil(w / 2)) bytes (`iter_yuv420(..., bits=10)` yields them; 16-bit arrays of half as many words are
    taken too).  "yuv444p10le", "gbrp10le" and "x2rgb10le" (10-bit 4:4:4: ProRes 4444 / DNxHR 444 decodes, image sequences, screen capture)
    are members of the same 10-bit family, in any pairing with it ("p010le" in with "x2rgb10le" out is allowed): UnpackDeep444 stands in
    front of the half chain and EgressDeep444 behind it (include/crtfx_444.h), items of `frame_iter` (`iter_deep444` yields them) and the
    arrays handed to `write_frame` are 1-D uint8 arrays of deep444.frame_bytes(h, w, fmt) bytes — 6 per pixel, 4 for x2rgb10le; 16-bit and
    32-bit arrays of the same bytes are taken too.  The matrix and range keywords apply to yuv444p10le; gbrp10le and x2rgb10le are
    full-range RGB and ignore them.  Refused with ValueError before a device is touched: a 10-bit format on one end only (the 8-bit stages have no half path,
    the 10-bit ones no uint8 path), `in_size` other than the output size (IngestResize has no half path), `resize_on="host"`.
    `in_chroma="left"` / `"center"` interpolates the chroma of a 4:2:0 / 4:2:2 input at that siting instead of replicating it over its
    pixels: UnpackSited (include/crtfx_sited.h) then stands where the family's source plan stood — in front of the half chain for
    "yuv420p10le" / "p010le", in front of IngestResize for an off-size 8-bit source.  "left" is the siting of MPEG-2 / H.264 / HEVC streams,
    "center" that of JPEG-family sources; "replicate" (default) is the path as it was.  Refused with ValueError before a device is touched:
    an unknown value, and "left" / "center" with "rgb24" or a 4:4:4 format (there is nothing to interpolate).
    `out_chroma="left"` filters the chroma of a 4:2:0 / 4:2:2 output onto the siting ffmpeg's muxers tag or assume (chroma_location=left:
    the sample on its first luma column, [1 2 1] / 4 around it) instead of writing the 2 x 2 / 2 x 1 box mean, which is centre siting:
    EgressSited (include/crtfx_egress_sited.h) then stands where the family's egress plan stood — behind the half chain for "yuv420p10le" /
    "p010le".  "center" (default) is the path as it was: the family's own plan, plan string and bytes.  Refused with ValueError before a
    device is touched: an unknown value, and "left" with "rgb24" or a 4:4:4 format (there is nothing to down-sample).
    `deliver_size=(dh, dw)` writes the frames at another size than they are rendered at (a 4K render delivered as 1080p: scanlines and the
    triad mask have periods of 2 and 3 pixels, and a render at the delivery resolution shows moire that a render at twice the size does not).
    The chain runs at out_h x out_w exactly as without it — text overlay, persistence state and grain are at render size; behind it the
    finished frames are resized on the device, uint8 ones by IngestResize (Pillow's BILINEAR bytes of the rendered frame), half ones by
    ResizeHalf (include/crtfx_resize16.h: the same resampler on quarter codes); behind that stands the egress plan of `out_pix_fmt`, built
    for (dh, dw).  The download and the arrays handed to `write_frame` have the delivery size (dh x dw x 3 for "rgb24", else
    frame_bytes(dh, dw) bytes).  `None` (default) and the render size itself are the path as it was: no resize plan is created.  Refused
    with ValueError before a device is touched: a value that is not a pair of integers, a size < 1 or > 32767.  (`in_size` for a 10-bit
    input stays refused: the source side of the half chain has no resize.)
    `in_filter` / `deliver_filter` name the filter of those two resizes, one of tables.RESAMPLE_FILTERS ("box", "bilinear", "hamming",
    "bicubic", "lanczos": Pillow's five).  "bilinear" (default) is the path as it was: IngestResize / ResizeHalf, their plan strings and
    bytes, and no Resample plan is created.  With another name Resample (include/crtfx_resample.h) stands where IngestResize stands for an
    off-size rgb24, 4:2:0 or 4:2:2 source, and where IngestResize or ResizeHalf stands behind the chain; uint8 frames come out as
    `Image.resize(size, filter)` gives them, and `resize_on="host"` hands `in_filter` to Pillow itself (the same bytes).  Refused with
    ValueError before a device is touched: an unknown name, and a `deliver_filter` other than "bilinear" without a `deliver_size` that
    differs from the render size (there is nothing to filter).
    `in_crop=(y, x, h, w)` cuts that window out of every source frame on the device before anything else sees it (a letterboxed film: the
    picture area, not the bars, fills the tube): Canvas (include/crtfx_canvas.h) stands behind the source plan and in front of the resize
    that brings the window to the render size.  With a packed `in_pix_fmt` it is a window of the `in_size` frame (of the render size
    without one); with "rgb24" a window of every frame at that frame's own size — a frame of the render size goes through it too — and a
    frame too small for it raises ValueError.  A 10-bit input may be cropped where the window has the render size (the Canvas then moves
    half pixels); any other window would have to be resized and is refused as `in_size` is.
    `deliver_fit` says how a render meets a `deliver_size` of another aspect: "stretch" (default) is the path as it was; "pad" resizes the
    render to the largest size of its own aspect inside the delivery (canvas.fit_pad) and centres it on a frame of `deliver_pad_color`
    (r, g, b in 0..255; a 4:3 render pillarboxed in 16:9); "crop" cuts the largest centred window of the delivery's aspect out of the
    render (canvas.fit_crop) and resizes that.  Where the aspects agree no Canvas is created and the bytes are those of "stretch".
    Refused with ValueError before a device is touched: an `in_crop` that is not four integers, has a side < 1 or leaves `in_size`;
    `in_crop` with `resize_on="host"`; an unknown `deliver_fit`; a `deliver_fit` other than "stretch" without a `deliver_size` that
    differs from the render size (there is nothing to fit); a pad colour outside 0..255.
    `chain_pix="half"` runs the chain on half pixels (FramePipeline(dtype=torch.float16)) whatever the formats, so the two ends need not
    have the same depth: a 10-bit master is delivered as "yuv420p" / "nv12", an 8-bit source is written as a 10-bit mezzanine, and an
    8-bit job gets the half chain, which rounds to 8 bits once, at the very end.  An 8-bit or "rgb24" source keeps its uint8 stages
    (source plan, Canvas, resize) and a Widen (include/crtfx_depth.h: half(u), exact) writes the chain's input behind them — an rgb24 frame
    at render size goes through a source end whose only stage is that Widen; an 8-bit or "rgb24" delivery runs its geometry (resize,
    Canvas) on the half frames, a Narrow at the delivery size turns them into uint8 frames, and the 8-bit egress plan reads those (for
    "rgb24" they are what is downloaded).  `dither` is that Narrow's rounding: "none" (default) rounds to nearest, ties to even, as the
    uint8 chain's quantiser does; "ordered" adds the 8 x 8 Bayer threshold of the pixel's place in the delivered frame before the floor,
    one threshold for the three channels, which breaks up the banding of smooth dark ramps (vignette, bloom).  A 10-bit end is as it was,
    with its refusals (`in_size`, a crop that needs a resize); with 10-bit formats on both ends "half" builds no depth plan and gives the
    bytes of "auto".  "auto" (default) is the path as it was, the one-end refusal included.  Refused with ValueError before a device is
    touched: an unknown `chain_pix` or `dither`; `dither` other than "none" where no Narrow would stand (`chain_pix="auto"`, or a 10-bit
    `out_pix_fmt`).
    `deinterlace="linear"` / `"edge"` takes every source frame as two fields woven into its even and odd rows (480i / 576i / 1080i tapes,
    consoles, camcorders, DVDs) and deinterlaces it on the device before anything else sees it: Deinterlace (include/crtfx_deint.h) stands
    directly behind the source plan, at the source size, in front of `in_crop`'s Canvas and the resize, which would mix the fields.  The
    rows of a field are kept; the rows between them are the rounded mean of the kept rows above and below ("linear") or of two pixels of
    those rows along the best of five directions, chosen per pixel ("edge").  `deinterlace="adaptive"` is motion-adaptive: an
    AdaptiveDeinterlace (include/crtfx_adeint.h) stands there instead, and the rows between are the OTHER field's own rows where the
    picture did not change since the previous source frame (still content keeps its full vertical resolution and does not bob under
    "both"), "edge"'s where it changed.  It is causal — the previous source frame, kept on the device across batches, is all it needs;
    the first frame of the stream, and the first frame behind a change of source size in a mixed rgb24 stream, has none and is "edge"'s.
    `field_order` "tff" (default) / "bff" says which field is the
    first.  `deinterlace_fields="first"` (default) writes one frame per source frame, made for the first field; `"both"` writes two, one per
    field in field order — a tube showed fields, not frames, and the persistence blend then decays field to field.  Under "both" a chain
    batch of B frames is fed by B // 2 source frames, B = `batch` taken even and at least 2; frame indices, `written`, `progress_cb` and
    the return value count frames WRITTEN (pass `total_frames` as such); the chain's clock stays `fps_out` as given: pass the FIELD rate
    (59.94 for 29.97i).  Every source then goes through a source end, as under `in_crop` or `chain_pix="half"` — an rgb24 frame at render
    size too — and an rgb24 frame of fewer than 2 rows raises ValueError.  "off" (default) is the path as it was: no Deinterlace is
    created.  Under every method the chroma rows of a 4:2:0 source are paired by its source plan as a progressive frame's are, in front of
    this stage, unless `in_chroma_rows="interlaced"` says that the fields were sub-sampled apart (below); 4:2:2, 4:4:4 and rgb24 sources
    have no such pairing.  Refused with ValueError before a device is touched: an unknown value of
    the three keywords; `field_order` or `deinterlace_fields` off its default with "off" (there is nothing to deinterlace);
    `resize_on="host"`; a source height below 2 where it is known (`in_size`, or the render size for a packed `in_pix_fmt`).
    `in_lut` / `deliver_lut` put a 3D colour LUT directly in front of the chain and directly behind it: a path to a `.cube` file or a
    `pythoncrt_amd.cube.Cube`, applied on the device with tetrahedral interpolation (Lut3D, include/crtfx_lut3d.h) at render size and on
    the chain's pixel type — what `lut3d=` in a second ffmpeg process did.  `in_lut` is the source end's last stage, behind the resize
    and behind the Widen of `chain_pix="half"`: a log-encoded camera source (ProRes 4444 / DNxHR 444 decodes) or an HDR10 one becomes
    display-referred video before the tube sees it, and an 8-bit log source on a half chain is transformed at half precision; every
    source then goes through a source end, an rgb24 frame at render size through one whose only stage is the LUT.  `deliver_lut` is the
    delivery end's first stage, in front of the delivery resize, the Canvas, the Narrow and the egress plan: a look or display
    transform on the finished frames; a pad colour is not transformed and the dither stays last.  HDR10 to SDR, with a PQ / BT.2020 ->
    BT.709 cube of the user's: `in_pix_fmt="p010le", in_lut="pq2020_to_709.cube"` (with `chain_pix="half"` for an 8-bit delivery).
    Stated limit: the cube's entries and the results are quarter codes (0..1020 for 0..255), so a cube's precision is 10 bits, and only the
    domain 0..1 and sizes 2..65 are taken.  `None` (default) creates no plan and no buffer: the path as it was.  Refused with ValueError
    before a device is touched: a cube that cannot be read or is malformed (the message names the file and the line), a value that is
    neither a path nor a Cube, and `in_lut` with `resize_on="host"`.
    `deliver_interlace="tff"` / `"bff"` delivers interlaced frames (1080i / 576i / 480i for DVD, broadcast, an interlaced encoder
    (`-flags +ilme+ildct`) or a real CRT): an Interlace (include/crtfx_interlace.h) weaves every two consecutive finished frames into one on
    the device, the first of a pair giving the even rows under "tff" and the odd rows under "bff" — what `interlace` / `tinterlace` in a
    second ffmpeg process did.  It is the delivery pair of `deinterlace_fields="both"`: a 29.97i source runs through the chain at field
    rate and leaves as 29.97i.  It stands at the DELIVERY size and on the chain's pixel type, behind the delivery resize and the Canvas (a
    vertical resize would mix the fields) and in front of the Narrow and the egress plan: the dither's coordinates are those of the
    delivered frame and the dither stays last.  `deliver_lowpass` filters every row vertically inside its own frame before the weave,
    against line twitter: "linear" is [1 2 1] / 4, "complex" [-1 2 6 2 -1] / 8 held back from over-sharpening; "none" (default) copies
    rows as bits.  The chain's batch B is `batch` taken even and at least 2, as under `deinterlace_fields="both"`, and a pair never
    straddles a batch: a batch with an odd frame count has its last frame woven with itself.  That happens at the end of the stream, and
    at a change of source size in a mixed rgb24 stream when no deinterlacer doubles the frames.  `written`, `progress_cb`, the return
    value and `total_frames` count DELIVERED frames; the chain's frame indices and its clock are unchanged: pass the field rate as
    `fps_out`.  "off" (default) builds no plan and no buffer: the path as it was.  The chroma rows of a 4:2:0 delivery are formed
    by the egress plan as a progressive frame's are, so they mix the two fields, unless `out_chroma_rows="interlaced"` is passed (below);
    4:2:2, 4:4:4 and rgb24 deliveries have no such pairing.  Refused with ValueError before a device is touched: an unknown value of either keyword; `deliver_lowpass` other than "none"
    with "off" (there is nothing to filter); a delivery height below 2.
    `in_signal="composite"` / `"svideo"` sends every source frame through the cable that fed the tube: a Signal (include/crtfx_signal.h)
    encodes every row to an NTSC-like signal and decodes it again on the device — colour that bleeds sideways and, under "composite", dot
    crawl on colour edges and rainbow fringes on fine luma detail; "svideo" keeps luma and chroma apart and only narrows the chroma — what
    a second ffmpeg or shader pass in front of this project did.  One pixel is one sample at 4 x fsc (four times the colour subcarrier,
    about 754 samples to an active line), so feed SD-width sources (`in_size`, or SD rgb24 frames); the resize to the render size is
    behind the stage.  It stands directly behind the source plan, at the source's own size and sample type, in front of the Deinterlace,
    `in_crop`'s Canvas, the resize, the Widen and `in_lut`: the cable carried the fields and the source's samples.  Every source then goes
    through a source end, as under `in_lut` — an rgb24 frame at render size through one whose only stage is the Signal.
    `signal_chroma` is the decoder's chroma low-pass, "sharp" (default: [1 2 3 4 3 2 1] / 16) or "soft" ([1 2 .. 8 .. 2 1] / 64);
    `signal_crawl` (default True) turns the subcarrier by 180 degrees per frame as well as per line, counted in SOURCE frames from the
    first one read, across changes of source size too.  "rgb" (default) builds no plan and no buffer: the path as it was.  Stated limits:
    NTSC-like only (no PAL, no burst-axis rotation, no RF noise); the rows of a woven interlaced frame are taken as consecutive lines; the
    chroma rows of a 4:2:0 source are formed in front of the stage by its source plan.  Refused with ValueError before a device is
    touched: an unknown value of the three keywords; `signal_chroma` or `signal_crawl` off its default with "rgb" (there is no signal);
    `resize_on="host"`.
    `in_chroma_rows="interlaced"` reads a 4:2:0 input ("yuv420p", "nv12", "yuv420p10le", "p010le") as an interlaced encoder wrote it
    (DVD, broadcast MPEG-2 and H.264 at 480i / 576i / 1080i, 10-bit HEVC at 1080i): chroma rows 0, 2, 4, ... belong to the top field and
    rows 1, 3, 5, ... to the bottom field, so every luma row takes its colour from rows of its own field — UnpackField420
    (include/crtfx_field420.h) then stands where the family's source plan or UnpackSited stood, at `in_chroma` ("replicate": the nearest
    chroma row of the field; "left" / "center": interpolated at MPEG-2's interlaced vertical siting and that horizontal siting).  Pass it
    with `deinterlace`: a deinterlacer, the Signal and the probe then read fields whose colour is their own, where under "progressive"
    (default: the path as it was) frame rows 4j + 1 and 4j + 2 carry the other field's colour and coloured motion combs in a way no
    deinterlacer can remove.  Refused with ValueError before a device is touched: an unknown value; "interlaced" with any other
    `in_pix_fmt`; a source height that is known (`in_size`, or the render size) and is odd or below 4.
    `out_chroma_rows="interlaced"` writes a 4:2:0 output ("yuv420p", "nv12", "yuv420p10le", "p010le") as an interlaced decoder reads it:
    chroma rows 0, 2, 4, ... are formed from the top field's luma rows and rows 1, 3, 5, ... from the bottom field's — EgressField420
    (include/crtfx_egress_field420.h) then stands where the family's egress plan or EgressSited stood, at `out_chroma` ("center": the box
    mean inside the field; "left": MPEG-2's interlaced vertical siting and that horizontal siting).  Pass it with `deliver_interlace`, or
    with a woven source that runs through undeinterlaced: under "progressive" (default: the path as it was) every chroma sample of such a
    frame is the mean of one row of each field, two moments apart, and colour combs on motion in every interlaced decoder.  With
    `in_chroma_rows="interlaced"`, `deinterlace_fields="both"` and `deliver_interlace` an interlaced 4:2:0 round trip stays on the device.
    Refused with ValueError before a device is touched: an unknown value; "interlaced" with any other `out_pix_fmt`; a delivered height
    (`deliver_size`, or the render size) that is no multiple of 4.
    `signal_standard="pal"` makes the cable of `in_signal` a PAL one — PAL DVD, DVB, PAL-region consoles and home computers, every 576i
    source: a PalSignal (include/crtfx_pal.h) stands in the Signal's place, with the same `signal_chroma` and `signal_crawl` and the same
    count of SOURCE frames.  Its subcarrier turns 270 degrees per line and per frame (only the index mod 4 matters) and the V axis switches
    sign every line.  `pal_decoder="delay"` (default) is the delay-line decoder: every line's chroma is averaged with the line above (row 0
    with row 1), which halves vertical chroma detail and turns a phase error into a loss of saturation; "simple" has no delay line, and a
    phase error then shows as Hanover bars — even and odd lines turn their hue opposite ways.  `signal_phase` is that error, the
    decoder's, in whole degrees -180..180 (default 0).  Pass it with `in_chroma_rows="interlaced"` for 576i 4:2:0.  "ntsc" (default)
    is the path as it was: the Signal with the keywords it had, and no PalSignal is created; NTSC has no phase knob.  Stated limits: the
    rows of a woven interlaced frame are taken as consecutive lines; no 25 Hz offset; no RF noise.  Refused with ValueError before a device
    is touched: an unknown value; a `signal_phase` that is a bool, no integer or outside -180..180; `pal_decoder` or `signal_phase` off
    its default under "ntsc"; "pal" with `in_signal="rgb"`.
    If `frame_iter` or `write_frame` raises, the GPU work already queued is drained (device synchronize) before the exception leaves this
    function, so that the staging buffers are not freed under a running copy."""
    import os
    import torch
    from .pipeline import FramePipeline, RenderSettings
    from .ends import StagingSlots
    from .options import ChainOptions, Raw
    unknown = set(io_keywords) - set(_IO_KEYS)
    if unknown:
        raise TypeError(f"process_frames() got unexpected keyword arguments {sorted(unknown)}")
    spec = ChainOptions.build(Raw(                                             # every refusal: options.RULES
        render_hw=(int(out_h), int(out_w)), resize_on=resize_on, out_pix_fmt=out_pix_fmt, out_matrix=out_matrix, out_range=out_range,
        in_pix_fmt=in_pix_fmt, in_matrix=in_matrix, in_range=in_range, in_size=in_size, in_chroma=in_chroma, out_chroma=out_chroma,
        deliver_size=deliver_size, in_filter=in_filter, deliver_filter=deliver_filter, in_crop=in_crop, deliver_fit=deliver_fit,
        deliver_pad_color=deliver_pad_color, chain_pix=chain_pix, dither=dither, deinterlace=deinterlace, field_order=field_order,
        deinterlace_fields=deinterlace_fields, in_lut=in_lut, deliver_lut=deliver_lut, deliver_interlace=deliver_interlace,
        deliver_lowpass=deliver_lowpass, in_signal=in_signal, signal_chroma=signal_chroma, signal_crawl=signal_crawl,
        in_chroma_rows=in_chroma_rows, out_chroma_rows=out_chroma_rows, signal_standard=signal_standard, pal_decoder=pal_decoder,
        signal_phase=signal_phase), "keywords")
    crop, ratio, deep = spec.crop, spec.ratio, formats.bits(in_pix_fmt) == 10
    if not torch.cuda.is_available():
        raise RuntimeError("no ROCm device visible; pythoncrt_amd has no CPU fallback")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    (h, w), (B, Bs) = spec.render_hw, spec.batch(batch)                        # the chain's batch, source frames per batch
    rs = RenderSettings(
        scanline_strength=float(scanline_strength), triad_strength=float(triad_strength), triad_gamma=float(triad_gamma),
        triad_preserve_luma=bool(triad_preserve_luma), triad_softness=float(triad_softness), aberration_px=int(aberration_px),
        bloom_sigma=float(bloom_sigma), bloom_strength=float(bloom_strength), bloom_threshold=float(bloom_threshold),
        noise_strength=float(noise_strength), vignette_strength=float(vignette_strength), persistence=float(persistence),
        scanline_speed_px_s=float(scanline_speed_px_s), scanline_period_px=float(scanline_period_px), fast_bloom=bool(fast_bloom),
        pixel_size=int(pixel_size), brightness=float(brightness), contrast=float(contrast), gamma=float(gamma), saturation=float(saturation),
        temperature=float(temperature), flicker_strength=float(flicker_strength), flicker_hz=float(flicker_hz), grain_size=int(grain_size),
        scanline_angle=float(scanline_angle), scanline_thickness=float(scanline_thickness), warp_strength=float(warp_strength),
        glitch_amp_px=int(glitch_amp_px), glitch_height_frac=float(glitch_height_frac))
    overlay = None
    if text:                                                                   # ref:1076-1077 (the same plane for every frame: built once)
        from .text import make_text_overlay_rgba
        overlay = make_text_overlay_rgba(w, h, text, text_font, int(text_size), text_color, tuple(text_pos))
    seed = int(noise_seed) if noise_seed is not None else int.from_bytes(os.urandom(8), "little")
    pix = torch.float16 if spec.half else torch.uint8                          # what the chain runs on
    pipe = FramePipeline(dev, h, w, rs, fps=float(fps_out), noise_seed=seed, dtype=pix, text_overlay_rgba=overlay, text_overlay_after=bool(text_after))
    total = max(1, int(total_frames)) if total_frames else None

    NS = 2
    pin_in = [torch.empty((B, h, w, 3), dtype=torch.uint8).pin_memory() for _ in range(NS)] if spec.direct else None   # else: a SourceEnd's own
    end = spec.delivery_end(dev, pix)
    pin_out = [torch.empty(end.shape(end.frames(B)), dtype=torch.uint8).pin_memory() for _ in range(NS)]    # what is downloaded and handed to the writer
    dev_in = [torch.empty((B, h, w, 3), dtype=pix, device=dev) for _ in range(NS)]
    dev_out = [torch.empty((B, h, w, 3), dtype=pix, device=dev) for _ in range(NS)]
    end.slots(dev_out)
    np_out = [t.numpy() for t in pin_out]
    compute, s_up, s_down = torch.cuda.current_stream(dev), torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    # rgb24 frames at render size are uploaded straight into dev_in.  Their kernels_done is the GLOBAL list: EVERY batch records its event there,
    # because every batch — an off-size one through its convert and the chain — reads dev_in[d]; an off-size source's own list covers ITS dev[d].
    direct = StagingSlots().adopt(dev_in, pin_in)
    down_done = [None] * NS          # the download that last read dev_out[d]
    state, index, written, k, pending = None, 0, 0, 0, None      # pending: (slot, frames, download event) of the batch still to be written

    MAX_SOURCES = 4                  # source sizes whose staging buffers and ingest plan are kept
    sources = {}                     # (src_h, src_w) -> SourceEnd, in order of last use
    last_key = None                  # the source key of the batch before: where it changes, a source that keeps a history starts a new one
    carry = None                     # a frame already taken from the iterator that starts the next batch (its source size differs)
    YUV = "yuv"                      # the key of the one 4:2:0 / 4:2:2 source (its size is fixed by in_size): a SourceEnd
    yuv_hw = spec.in_size or (h, w)
    yuv_bytes = formats.frame_bytes(yuv_hw[0], yuv_hw[1], in_pix_fmt)

    def source(key):
        src = sources.pop(key, None)
        if src is None:
            if len(sources) >= MAX_SOURCES:      # rare: drop the least recently used size once its queued work is done
                torch.cuda.synchronize(dev)
                sources.pop(next(iter(sources)))
            src = spec.source_end(dev, yuv_hw if key == YUV else key, pix).slots(Bs, NS)
            assert key != YUV or src.frame_bytes == yuv_bytes
        sources[key] = src
        return src

    def fit(frame):
        """(array to stage, None) for a frame at the output size or resized on the host; (array, (src_h, src_w)) for one the device resizes."""
        a = np.asarray(frame)
        if in_pix_fmt != "rgb24":
            a = a.reshape(-1)
            if deep and a.dtype.itemsize in (2, 4):  # 16-bit (or x2rgb10le's 32-bit) words: the same bytes
                a = np.ascontiguousarray(a).view(np.uint8)
            if a.size != yuv_bytes:
                raise ValueError(f"a {in_pix_fmt} frame of {yuv_hw[0]} x {yuv_hw[1]} holds {yuv_bytes} bytes, got an item of {a.size}")
            return a, YUV
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"frames must be H x W x 3 RGB arrays, got {a.shape}")
        if spec.deinterlace is not None and a.shape[0] < 2:
            raise ValueError(f"deinterlace={deinterlace!r}: a frame of {a.shape[0]} x {a.shape[1]} has no two fields")
        if crop is not None:                                                    # every frame goes through a SourceEnd of ITS size
            if a.shape[0] < crop[0] + crop[2] or a.shape[1] < crop[1] + crop[3]:
                raise ValueError(f"in_crop={crop}: the window leaves a frame of {a.shape[0]} x {a.shape[1]}")
            return a, (int(a.shape[0]), int(a.shape[1]))
        if a.shape[0] != h or a.shape[1] != w:                                  # ref:1039-1041
            if resize_on == "device":
                return a, (int(a.shape[0]), int(a.shape[1]))
            from PIL import Image
            a = np.asarray(Image.fromarray(np.ascontiguousarray(a, dtype=np.uint8)).resize((w, h), getattr(Image, in_filter.upper())))
        return a, (None if spec.direct else (h, w))      # a half chain, a deinterlaced source, an in_lut, an in_signal: no direct upload, the frame goes through a source end

    def drain(p):
        nonlocal written
        d, n, ev = p
        ev.synchronize()
        for j in range(n):
            write_frame(np_out[d][j])                                           # ref:1101
            written += 1
            if progress_cb is not None and total:
                progress_cb(min(1.0, written / float(total)))                   # ref:1104-1105

    try:
        it = iter(frame_iter)
        done = False
        while not done:
            d = k % NS
            n, key, src = 0, None, None
            while n < Bs:
                if carry is not None:
                    (a, akey), carry = carry, None
                else:
                    try:
                        frame = next(it)
                    except StopIteration:
                        done = True
                        break
                    a, akey = fit(frame)
                if n == 0:
                    key, src = akey, direct if akey is None else source(akey)      # an off-size batch is staged at ITS size
                    if src.up_done[d] is not None:
                        src.up_done[d].synchronize()     # the upload that read this pinned slot two batches ago (long done)
                    slot = src.np[d]
                elif akey != key:                        # the source size changes: this frame opens the next batch
                    carry = (a, akey)
                    break
                np.copyto(slot[n], a, casting="unsafe")
                n += 1
            if n:
                if src.kernels_done[d] is not None:      # the kernels that last read src.dev[d]: for `direct`, those of whichever batch came last
                    s_up.wait_event(src.kernels_done[d])
                with torch.cuda.stream(s_up):
                    src.dev[d][:n].copy_(src.pin[d][:n], non_blocking=True)
                    up = torch.cuda.Event()
                    up.record(s_up)
                src.up_done[d] = up
                compute.wait_event(up)
                # dev_in[d]: its last upload (two batches ago) was awaited by `compute` then, its last readers ran on `compute`
                m = n * ratio                        # the frames the chain runs: n source frames, `ratio` each
                md = end.frames(m)                   # the frames the writer gets: m, or ceil(m / 2) woven ones
                if key != last_key and src is not direct:
                    src.restart()                    # deinterlace="adaptive": the frame before this batch's first is not its previous frame
                last_key = key
                if spec.signal is not None:
                    src.index = index // ratio       # the batch's first SOURCE frame in the stream: the Signal's t
                src.convert(d, n, dev_in[d][:m])                                     # on the compute stream; nothing for `direct`
                if down_done[d] is not None:
                    compute.wait_event(down_done[d])
                _, state = pipe.run(dev_in[d][:m], first_index=index, state=state, out=dev_out[d][:m])
                send = end.run(d, m)                 # behind the chain on the compute stream; the slot's last download was awaited above
                kd = torch.cuda.Event()
                kd.record(compute)
                direct.kernels_done[d] = src.kernels_done[d] = kd      # the kernels that last read dev_in[d] / wrote dev_out[d]
                # pin_out[d] was drained one iteration ago (drain below runs before the next batch is enqueued into the same slot)
                s_down.wait_event(kd)
                with torch.cuda.stream(s_down):
                    pin_out[d][:md].copy_(send, non_blocking=True)
                    dn = torch.cuda.Event()
                    dn.record(s_down)
                down_done[d] = dn
                index += m
            # the PREVIOUS batch's frames go to the writer while this batch is on the GPU
            if pending is not None:
                drain(pending)
                pending = None
            if n:
                pending = (d, md, dn)
            k += 1
        if pending is not None:
            drain(pending)
    except BaseException:
        with contextlib.suppress(Exception):     # the caller's exception is the one to report
            torch.cuda.synchronize(dev)          # uploads / kernels / downloads still in flight reference the buffers above
        raise
    if progress_cb is not None and not total:
        progress_cb(1.0)
    return written
