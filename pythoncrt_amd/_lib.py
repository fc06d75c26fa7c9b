"""ctypes binding of libcrtfx.so (include/crtfx.h).  No torch types cross this boundary:
pointers are integers (tensor.data_ptr()), sizes are ints.  Missing library = hard error —
there is no CPU fallback in the product path."""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("CRTFX_LIB") or os.path.join(_HERE, "libcrtfx.so")   # CRTFX_LIB: dev A/B builds only
CSRC = os.path.join(_HERE, "csrc")
SOURCES = [os.path.join(CSRC, f) for f in ("crtfx.hip", "crtfx_rr.hip", "crtfx_kernels.hip.h", "crtfx_common.hip.h", "crtfx_blur.hip.h", "crtfx_point.hip.h",
                                                "crtfx_phosphor.hip.h", "crtfx_phosphor_ct.hip.h", "crtfx_warp.hip.h", "crtfx_internal.h", "crtfx_ingest.hip",
                                                "crtfx_egress.hip", "crtfx_unpack.hip", "crtfx_deep.hip", "crtfx_422.hip", "crtfx_444.hip", "crtfx_sited.hip", "crtfx_egress_sited.hip", "crtfx_field420.hip", "crtfx_egress_field420.hip", "crtfx_resize16.hip", "crtfx_resample.hip", "crtfx_canvas.hip", "crtfx_depth.hip", "crtfx_deint.hip", "crtfx_adeint.hip", "crtfx_edge.hip.h", "crtfx_lut3d.hip", "crtfx_interlace.hip", "crtfx_signal.hip", "crtfx_pal.hip", "crtfx_probe.hip", "crtfx_stage_host.h", "crtfx_resize_host.h", "crtfx_frame_host.h")] + \
          [os.path.join(ROOT, "include", f) for f in ("crtfx.h", "crtfx_ingest.h", "crtfx_egress.h", "crtfx_unpack.h", "crtfx_deep.h", "crtfx_422.h", "crtfx_444.h", "crtfx_sited.h", "crtfx_egress_sited.h", "crtfx_field420.h", "crtfx_egress_field420.h", "crtfx_resize16.h", "crtfx_resample.h", "crtfx_canvas.h", "crtfx_depth.h", "crtfx_deint.h", "crtfx_adeint.h", "crtfx_lut3d.h", "crtfx_interlace.h", "crtfx_signal.h", "crtfx_pal.h", "crtfx_probe.h")]
STAGE_UNITS = ("crtfx_ingest", "crtfx_egress", "crtfx_unpack", "crtfx_deep", "crtfx_422", "crtfx_444", "crtfx_sited", "crtfx_egress_sited", "crtfx_field420", "crtfx_egress_field420", "crtfx_resize16", "crtfx_resample", "crtfx_canvas", "crtfx_depth", "crtfx_deint", "crtfx_adeint", "crtfx_lut3d", "crtfx_interlace", "crtfx_signal", "crtfx_pal", "crtfx_probe")   # one object file each, beside crtfx.hip / crtfx_rr.hip
RR_RADII = tuple(range(1, 31))      # one register-window build per radius up to 30 (crtfx_internal.h); larger radii: the split path

OK, E_INVALID, E_HIP, E_UNSUPPORTED, E_NOMEM = 0, -1, -2, -3, -4
PIX_U8, PIX_F16 = 0, 1
BLEND_NONE, BLEND_RENDER, BLEND_PREVIEW = 0, 1, 2

F_SATURATION, F_TEMPERATURE, F_BRIGHTCON, F_GAMMA = 1 << 0, 1 << 1, 1 << 2, 1 << 3
F_BLOOM, F_BLOOM_FAST, F_BLOOM_THR = 1 << 4, 1 << 5, 1 << 6
F_TRIAD, F_TRIAD_LUT, F_TRIAD_LUMA = 1 << 7, 1 << 8, 1 << 9
F_SCANLINES, F_VIGNETTE, F_FLICKER, F_NOISE, F_WARP, F_PIXELATE = 1 << 10, 1 << 11, 1 << 12, 1 << 13, 1 << 14, 1 << 15

_vp = ctypes.c_void_p


class CrtfxParams(ctypes.Structure):
    _fields_ = [
        ("size", ctypes.c_uint32), ("flags", ctypes.c_uint32),
        ("aberration_px", ctypes.c_int32), ("grain_size", ctypes.c_int32),
        ("bloom_radius", ctypes.c_int32), ("reserved0", ctypes.c_int32),
        ("saturation", ctypes.c_float), ("r_gain", ctypes.c_float), ("b_gain", ctypes.c_float),
        ("contrast", ctypes.c_float), ("brightness", ctypes.c_float), ("inv_gamma", ctypes.c_float),
        ("bloom_thr", ctypes.c_float), ("bloom_thr_den", ctypes.c_float), ("bloom_strength", ctypes.c_float),
        ("noise_scale", ctypes.c_float), ("warp_k", ctypes.c_float), ("warp_cx", ctypes.c_float), ("warp_cy", ctypes.c_float),
        ("vignette_strength", ctypes.c_double),
        ("bloom_taps", _vp), ("triad_row", _vp), ("lut_g", _vp), ("lut_inv", _vp),
        ("vig_nx2", _vp), ("vig_ny2", _vp), ("warp_xhat", _vp), ("warp_yhat", _vp),
        ("pix_xmap", _vp), ("pix_ymap", _vp),
        ("triad_full_dev", _vp), ("vignette_full_dev", _vp),
        ("grain_xofs", _vp), ("grain_xw", _vp), ("grain_yofs", _vp), ("grain_yw", _vp),
        ("grain_w", ctypes.c_int32), ("grain_h", ctypes.c_int32),
        ("fbu_xofs", _vp), ("fbu_xw", _vp), ("fbu_yofs", _vp), ("fbu_yw", _vp),
        ("fbd_xofs", _vp), ("fbd_xw", _vp), ("fbd_yofs", _vp), ("fbd_yw", _vp),
        ("grade_lut", _vp),
    ]


class CrtfxFrame(ctypes.Structure):
    _fields_ = [
        ("scan_row_dev", _vp), ("scan_plane_dev", _vp), ("noise_plane_dev", _vp),
        ("overlay_rgba_dev", _vp), ("glitch_offs_dev", _vp),
        ("flicker_factor", ctypes.c_double), ("noise_seed", ctypes.c_uint64), ("frame_index", ctypes.c_uint64),
        ("overlay_after", ctypes.c_int32), ("glitch_y0", ctypes.c_int32), ("glitch_cols", ctypes.c_int32),
        ("glitch_seg_len", ctypes.c_int32),
    ]


# name -> (restype, argtypes); every symbol include/crtfx.h declares
SYMBOLS = {
    "crtfx_version": (ctypes.c_int, []),
    "crtfx_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp)]),
    "crtfx_destroy": (ctypes.c_int, [_vp]),
    "crtfx_last_error": (ctypes.c_char_p, [_vp]),
    "crtfx_set_params": (ctypes.c_int, [_vp, ctypes.POINTER(CrtfxParams)]),
    "crtfx_apply_static": (ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(CrtfxFrame), _vp]),
    "crtfx_apply": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_double, ctypes.POINTER(CrtfxFrame), _vp]),
    "crtfx_blend_quantise": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_double, _vp]),
    "crtfx_halo_correct_quantise": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_double, _vp, _vp, _vp]),
    "crtfx_process_batch": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int,
                                           ctypes.POINTER(CrtfxFrame), _vp, ctypes.c_double, ctypes.c_int, _vp, _vp]),
    "crtfx_noise_plane": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _vp, _vp]),
    "crtfx_halo_correct_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_double, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_size_t, _vp]),
    "crtfx_warp_map": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "crtfx_resize_state": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp]),
    "crtfx_scanline_plane": (ctypes.c_int, [_vp] + [ctypes.c_double] * 5 + [_vp, _vp]),
    "crtfx_set_option": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "crtfx_debug_buffer": (ctypes.c_int, [_vp, _vp]),
    "crtfx_profile_enable": (ctypes.c_int, [_vp, ctypes.c_int]),
    "crtfx_profile_read": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "crtfx_last_plan": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t]),
    "crtfx_kernel_lds_bytes": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.c_int]),
    "crtfx_host_blur_row": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int]),
}

def resize_symbols(*families):
    """The six entry points of each crtfx_<family>_* family of resize stages (include/crtfx_ingest.h spells them out; pythoncrt_amd/_stage.py
    is their one caller)."""
    return {f"crtfx_{fam}_{name}": sig for fam in families for name, sig in (
        ("create", (ctypes.c_int, [ctypes.c_int] * 6 + [_vp, _vp, _vp, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int, ctypes.POINTER(_vp)])),
        ("destroy", (ctypes.c_int, [_vp])),
        ("last_error", (ctypes.c_char_p, [_vp])),
        ("run", (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp])),
        ("set_option", (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int])),
        ("last_plan", (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t])))}


# ... and every symbol include/crtfx_ingest.h declares (the ingest stage: a handle of its own, pythoncrt_amd/ingest.py)
INGEST_OPT_FORCE_GENERAL = 1
INGEST_SYMBOLS = resize_symbols("ingest")


def stage_symbols(*families):
    """The seven entry points of each crtfx_<family>_* family of format stages (include/crtfx_egress.h spells them out; pythoncrt_amd/_stage.py
    is their one caller)."""
    return {f"crtfx_{fam}_{name}": sig for fam in families for name, sig in (
        ("create", (ctypes.c_int, [ctypes.c_int] * 5 + [_vp, _vp, ctypes.POINTER(_vp)])),
        ("destroy", (ctypes.c_int, [_vp])),
        ("last_error", (ctypes.c_char_p, [_vp])),
        ("frame_bytes", (ctypes.c_size_t, [_vp])),
        ("run", (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp])),
        ("set_option", (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int])),
        ("last_plan", (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t])))}


# ... and every symbol include/crtfx_egress.h declares (the egress stage: a handle of its own, pythoncrt_amd/egress.py)
EGRESS_YUV420P, EGRESS_NV12 = 0, 1
EGRESS_OPT_FORCE_GENERAL = 1
EGRESS_SYMBOLS = stage_symbols("egress")

# ... and every symbol include/crtfx_unpack.h declares (the source stage: a handle of its own, pythoncrt_amd/unpack.py)
UNPACK_YUV420P, UNPACK_NV12 = 0, 1
UNPACK_OPT_FORCE_GENERAL = 1
UNPACK_SYMBOLS = stage_symbols("unpack")

# ... and every symbol include/crtfx_deep.h declares (the 10-bit source and egress stages: two handle families, pythoncrt_amd/deep.py)
DEEP_YUV420P10LE, DEEP_P010LE = 0, 1
UNPACK10_OPT_FORCE_GENERAL = 1
EGRESS10_OPT_FORCE_GENERAL = 1
DEEP_SYMBOLS = stage_symbols("unpack10", "egress10")

# ... and every symbol include/crtfx_422.h declares (the 8-bit 4:2:2 source and egress stages: two handle families, pythoncrt_amd/yuv422.py)
YUV422_YUV422P, YUV422_YUYV422, YUV422_UYVY422 = 0, 1, 2
UNPACK422_OPT_FORCE_GENERAL = 1
EGRESS422_OPT_FORCE_GENERAL = 1
YUV422_SYMBOLS = stage_symbols("unpack422", "egress422")

# ... and every symbol include/crtfx_444.h declares (the 10-bit 4:4:4 source and egress stages: two handle families, pythoncrt_amd/deep444.py)
DEEP444_PLANAR, DEEP444_X2RGB10LE = 0, 1
UNPACK444_OPT_FORCE_GENERAL = 1
EGRESS444_OPT_FORCE_GENERAL = 1
DEEP444_SYMBOLS = stage_symbols("unpack444", "egress444")

# ... and every symbol include/crtfx_sited.h declares (the sited source stage of the seven sub-sampled formats: one handle family, pythoncrt_amd/sited.py)
SITED_YUV420P, SITED_NV12, SITED_YUV422P, SITED_YUYV422, SITED_UYVY422, SITED_YUV420P10LE, SITED_P010LE = range(7)
SITED_LEFT, SITED_CENTER = 0, 1
SITED_OPT_FORCE_GENERAL, SITED_OPT_SITING = 1, 2
SITED_SYMBOLS = stage_symbols("sited")

# ... and every symbol include/crtfx_egress_sited.h declares (the sited egress stage of the same seven formats, with the layout and siting numbers
# above: one handle family, pythoncrt_amd/sited.py)
EGRESS_SITED_OPT_FORCE_GENERAL, EGRESS_SITED_OPT_SITING = 1, 2
EGRESS_SITED_SYMBOLS = stage_symbols("egress_sited")

# ... and every symbol include/crtfx_field420.h declares (the field-paired 4:2:0 source stage, for interlaced sources: one handle family,
# pythoncrt_amd/field420.py)
FIELD420_YUV420P, FIELD420_NV12, FIELD420_YUV420P10LE, FIELD420_P010LE = range(4)
FIELD420_REPLICATE, FIELD420_LEFT, FIELD420_CENTER = 0, 1, 2
FIELD420_OPT_FORCE_GENERAL, FIELD420_OPT_CHROMA = 1, 2
FIELD420_SYMBOLS = stage_symbols("field420")

# ... and every symbol include/crtfx_egress_field420.h declares (the field-paired 4:2:0 egress stage, for interlaced deliveries, with the
# layout numbers above: one handle family, pythoncrt_amd/field420.py)
EGRESS_FIELD420_CENTER, EGRESS_FIELD420_LEFT = 0, 1
EGRESS_FIELD420_OPT_FORCE_GENERAL, EGRESS_FIELD420_OPT_CHROMA = 1, 2
EGRESS_FIELD420_SYMBOLS = stage_symbols("egress_field420")

# ... and every symbol include/crtfx_resize16.h declares (the half resampler: a handle of its own, pythoncrt_amd/resize16.py; the shape of the
# ingest stage's table)
RESIZE16_OPT_FORCE_GENERAL = 1
RESIZE16_SYMBOLS = resize_symbols("resize16")

# ... and every symbol include/crtfx_resample.h declares (the filtered resampler, uint8 and half: a handle of its own, pythoncrt_amd/resample.py;
# the shape of the ingest stage's table)
RESAMPLE_OPT_FORCE_GENERAL, RESAMPLE_OPT_ACC64 = 1, 2
RESAMPLE_SYMBOLS = resize_symbols("resample")

def frame_symbols(family, create_args, **extra):
    """The six entry points of one crtfx_<family>_* family of frame stages (RGB frames to RGB frames; pythoncrt_amd/_stage.py's FramePlan is
    their caller): a create of the family's own — device, create_args..., &plan — the five every family spells the same way, and what `extra`
    names: a further entry point, or the family's own signature of one of the five."""
    table = {"create": (ctypes.c_int, [ctypes.c_int, *create_args, ctypes.POINTER(_vp)]),
             "destroy": (ctypes.c_int, [_vp]),
             "last_error": (ctypes.c_char_p, [_vp]),
             "run": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
             "set_option": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
             "last_plan": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t]),
             **extra}
    return {f"crtfx_{family}_{name}": sig for name, sig in table.items()}


_FRAMES_OUT = (ctypes.c_int, [_vp])

# ... and every symbol include/crtfx_canvas.h declares (the geometry stage, uint8 and half: a handle of its own, pythoncrt_amd/canvas.py; its
# create: device, pix_fmt, src_h, src_w, win_y, win_x, win_h, win_w, dst_h, dst_w, dst_y, dst_x, fill[3], &plan)
CANVAS_OPT_FORCE_GENERAL = 1
CANVAS_SYMBOLS = frame_symbols("canvas", [ctypes.c_int] * 11 + [ctypes.POINTER(ctypes.c_uint16)])

# ... and every symbol include/crtfx_depth.h declares (the depth stage, uint8 <-> half: a handle of its own, pythoncrt_amd/depth.py; its
# create: device, h, w, direction, dither, &plan)
DEPTH_WIDEN, DEPTH_NARROW = 0, 1
DITHER_NONE, DITHER_ORDERED = 0, 1
DEPTH_OPT_FORCE_GENERAL = 1
DEPTH_SYMBOLS = frame_symbols("depth", [ctypes.c_int] * 4)

# ... and every symbol include/crtfx_deint.h declares (the deinterlace stage, uint8 and half: a handle of its own, pythoncrt_amd/deint.py; its
# create — device, h, w, pix_fmt, method, order, fields, &plan — and frames_out)
DEINT_LINEAR, DEINT_EDGE = 0, 1
DEINT_TFF, DEINT_BFF = 0, 1
DEINT_FIRST, DEINT_BOTH = 0, 1
DEINT_OPT_FORCE_GENERAL = 1
DEINT_SYMBOLS = frame_symbols("deint", [ctypes.c_int] * 6, frames_out=_FRAMES_OUT)

# ... and every symbol include/crtfx_adeint.h declares (the motion-adaptive deinterlace stage, uint8 and half: a handle of its own,
# pythoncrt_amd/adeint.py; a create without a method — device, h, w, pix_fmt, order, fields, &plan — frames_out, and a run that takes the
# previous frame first; the order and field numbers are DEINT_*)
ADEINT_OPT_FORCE_GENERAL = 1
ADEINT_SYMBOLS = frame_symbols("adeint", [ctypes.c_int] * 5, frames_out=_FRAMES_OUT,
                               run=(ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp]))

# ... and every symbol include/crtfx_lut3d.h declares (the 3D LUT stage, uint8 and half: a handle of its own, pythoncrt_amd/lut3d.py; its
# create — device, h, w, pix_fmt, N, table, &plan — and set_table)
LUT3D_QMAX, LUT3D_MIN_N, LUT3D_MAX_N, LUT3D_LDS_MAX_N = 1020, 2, 65, 34
LUT3D_OPT_FORCE_GENERAL, LUT3D_OPT_FORCE_GLOBAL = 1, 2
LUT3D_SYMBOLS = frame_symbols("lut3d", [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_uint16)],
                              set_table=(ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint16)]))

# ... and every symbol include/crtfx_interlace.h declares (the interlace stage, uint8 and half: a handle of its own, pythoncrt_amd/interlace.py;
# its create — device, h, w, pix_fmt, order, lowpass, &plan — and frames_in)
INTERLACE_TFF, INTERLACE_BFF = 0, 1
INTERLACE_NONE, INTERLACE_LINEAR, INTERLACE_COMPLEX = 0, 1, 2
INTERLACE_OPT_FORCE_GENERAL = 1
INTERLACE_SYMBOLS = frame_symbols("interlace", [ctypes.c_int] * 5, frames_in=_FRAMES_OUT)

# ... and every symbol include/crtfx_signal.h declares (the composite-video stage, uint8 and half: a handle of its own, pythoncrt_amd/signal.py;
# its create — device, h, w, pix_fmt, signal, chroma, crawl, &plan — and a run that takes the first frame's index in the stream first)
SIGNAL_COMPOSITE, SIGNAL_SVIDEO = 0, 1
SIGNAL_SHARP, SIGNAL_SOFT = 0, 1
SIGNAL_OPT_FORCE_GENERAL = 1
SIGNAL_SYMBOLS = frame_symbols("signal", [ctypes.c_int] * 6,
                               run=(ctypes.c_int, [_vp, ctypes.c_int64, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp]))

# ... and every symbol include/crtfx_pal.h declares (the PAL composite-video stage, uint8 and half: a handle of its own, pythoncrt_amd/pal.py;
# its create — device, h, w, pix_fmt, signal, chroma, crawl, decoder, phase, &plan — a run that takes the first frame's index in the stream
# first, as the signal stage's, and phase_table, which needs no plan; the signal and chroma numbers are SIGNAL_*)
PAL_DELAY, PAL_SIMPLE = 0, 1
PAL_OPT_FORCE_GENERAL = 1
PAL_SYMBOLS = frame_symbols("pal", [ctypes.c_int] * 8,
                            run=(ctypes.c_int, [_vp, ctypes.c_int64, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
                            phase_table=(ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]))

# ... and every symbol include/crtfx_probe.h declares (the source probe, uint8 and half: a handle of its own, pythoncrt_amd/probe.py; its
# create — device, h, w, pix_fmt, &plan — a run that takes the previous frame first, as adeint's, and writes records, and words, which needs no plan)
PROBE_OPT_FORCE_GENERAL = 1
PROBE_SYMBOLS = frame_symbols("probe", [ctypes.c_int] * 3,
                              run=(ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
                              words=(ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]))

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC"]


def build(force: bool = False, verbose: bool = False, extra_flags=(), out: str = None) -> str:
    """Compile libcrtfx.so in-tree for gfx950 (hipcc cross-compiles without a GPU): crtfx.hip plus
    crtfx_rr.hip once per radius, the translation units in parallel, then one link."""
    out = out or LIB_PATH
    if not force and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in SOURCES):
        return out
    from concurrent.futures import ThreadPoolExecutor
    hipcc = "hipcc" if _which("hipcc") else "/opt/rocm/bin/hipcc"
    objdir = os.path.join(ROOT, "build", "obj", os.path.basename(out))
    os.makedirs(objdir, exist_ok=True)
    inc = ["-I", os.path.join(ROOT, "include"), "-I", CSRC]
    jobs = [([hipcc, *HIPCC_FLAGS, *extra_flags, *inc, "-c", os.path.join(CSRC, "crtfx.hip"), "-o", os.path.join(objdir, "crtfx.o")])]
    for r in RR_RADII:
        jobs.append([hipcc, *HIPCC_FLAGS, *extra_flags, *inc, f"-DRR_R={r}", "-c", os.path.join(CSRC, "crtfx_rr.hip"),
                     "-o", os.path.join(objdir, f"crtfx_rr_{r}.o")])
    for unit in STAGE_UNITS:
        jobs.append([hipcc, *HIPCC_FLAGS, *extra_flags, *inc, "-c", os.path.join(CSRC, unit + ".hip"), "-o", os.path.join(objdir, unit + ".o")])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL if not verbose else None)

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 4)) as ex:
        list(ex.map(run, jobs))
    objs = [j[-1] for j in jobs]
    run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out, *objs])
    return out


def build_variant(name: str, extra_flags, radii=(9,), main_tu: bool = False) -> str:
    """Dev A/B builds (tools/ab.sh; never the product library): build/ab/libcrtfx_<name>.so = the in-tree library's objects with the
    translation units of `radii` (and crtfx.hip when main_tu) recompiled with extra_flags.  Load one with CRTFX_LIB=<path>."""
    build()
    hipcc = "hipcc" if _which("hipcc") else "/opt/rocm/bin/hipcc"
    base = os.path.join(ROOT, "build", "obj", os.path.basename(LIB_PATH))
    objdir = os.path.join(ROOT, "build", "obj", f"ab_{name}")
    os.makedirs(objdir, exist_ok=True)
    os.makedirs(os.path.join(ROOT, "build", "ab"), exist_ok=True)
    inc = ["-I", os.path.join(ROOT, "include"), "-I", CSRC]
    objs = []
    for r in RR_RADII:
        o = os.path.join(base, f"crtfx_rr_{r}.o")
        if r in radii:
            o = os.path.join(objdir, f"crtfx_rr_{r}.o")
            subprocess.run([hipcc, *HIPCC_FLAGS, *extra_flags, *inc, f"-DRR_R={r}", "-c", os.path.join(CSRC, "crtfx_rr.hip"), "-o", o], check=True)
        objs.append(o)
    main = os.path.join(base, "crtfx.o")
    if main_tu:
        main = os.path.join(objdir, "crtfx.o")
        subprocess.run([hipcc, *HIPCC_FLAGS, *extra_flags, *inc, "-c", os.path.join(CSRC, "crtfx.hip"), "-o", main], check=True)
    out = os.path.join(ROOT, "build", "ab", f"libcrtfx_{name}.so")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out, main, *objs,
                    *(os.path.join(base, unit + ".o") for unit in STAGE_UNITS)], check=True)
    return out


def _which(name):
    from shutil import which
    return which(name)


_LIB = None


def load() -> ctypes.CDLL:
    """dlopen the in-tree libcrtfx.so and type every entry point.  Raises if it is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or pythoncrt_amd._lib.build()). "
            "pythoncrt_amd has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in {**SYMBOLS, **INGEST_SYMBOLS, **EGRESS_SYMBOLS, **UNPACK_SYMBOLS, **DEEP_SYMBOLS, **YUV422_SYMBOLS, **DEEP444_SYMBOLS,
                               **SITED_SYMBOLS, **EGRESS_SITED_SYMBOLS, **FIELD420_SYMBOLS, **EGRESS_FIELD420_SYMBOLS, **RESIZE16_SYMBOLS, **RESAMPLE_SYMBOLS, **CANVAS_SYMBOLS, **DEPTH_SYMBOLS, **DEINT_SYMBOLS, **ADEINT_SYMBOLS, **LUT3D_SYMBOLS, **INTERLACE_SYMBOLS, **SIGNAL_SYMBOLS, **PAL_SYMBOLS, **PROBE_SYMBOLS}.items():
        fn = getattr(lib, name)   # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    if lib.crtfx_version() != 1:
        raise RuntimeError(f"libcrtfx ABI {lib.crtfx_version()} != 1")
    _LIB = lib
    return lib


class CrtfxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libcrtfx error {code}: {msg}")
        self.code = code


def check(lib, ctx, rc):
    if rc != OK:
        msg = lib.crtfx_last_error(ctx)
        raise CrtfxError(rc, msg.decode() if msg else "")
