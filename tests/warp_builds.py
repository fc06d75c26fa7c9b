"""The warp / commit kernel builds and how each one is reached: the table that drives tests/test_warp_builds_gpu.py (every build held to the
float32-storage model tests/warp_model.py on the GPU, bit for bit) and the CPU inventory in tests/test_evidence_tools.py (every k_warp_lean /
k_warp instance in the library has a row).  No torch import here.

The launcher (crtfx.hip launch_warp_group / launch_warp_lean2) can reach 32 k_warp_lean instances — {f32, f64} x {none, render} x {u8, half}
x rows {1, 2, 4} of the general build, six branch-free `plain` builds and two commit-only builds — and the general k_warp (gather and
commit-only are one instance: `identity` is a run-time argument).

A row names its kernel instance (template arguments as the demangler prints them), the route that reaches it, the chain dtype (f32: no
vignette / flicker; f64: promoted), the blend, the pixel format, the DEBUG_OPTIONS, the widths it is reachable on and the exact
crtfx_last_plan `warp=` string it must produce.  Routes:

  loop      FramePipeline.run (crtfx_process_batch): warp on; blend none = persistence 0, render = a persistence chain;
  commit    FramePipeline.run with the warp OFF behind the Gaussian chain and a persistence chain: the commit-only build;
  api       apply_static_effects: one frame, its float image (never lean: a float output takes the general k_warp);
  preview   apply_crt_effect ticks threaded through state_prev (cv2.addWeighted blend: the general k_warp)."""
from dataclasses import dataclass, field

BLEND = {"none": 0, "render": 1}
PIX = {"u8": 0, "half": 1}


def lean_instance(prom, blend, pix, rows, ident=False, plain=False):
    """crtfx::k_warp_lean<PROMOTE, BLEND, PIX, ROWS, IDENT, WX, SEQ, PLAIN> as tools/kernel_resources.resources names it: unblended frames
    run two waves side by side (WX = 2), one frame per thread (SEQ false); a persistence chain WX = 1, its frames in sequence."""
    b = lambda v: "true" if v else "false"      # noqa: E731
    wx, seq = (1, True) if blend == "render" else (2, False)
    return f"crtfx::k_warp_lean<{b(prom)}, {BLEND[blend]}, {PIX[pix]}, {rows}, {b(ident)}, {wx}, {b(seq)}, {b(plain)}>"


def lean_plan(chain, blend, pix, rows, plain=False):
    tile = f"64x{4 * rows}" if blend == "render" else f"128x{2 * rows}"
    return f"k_warp_lean<{chain},{blend},{pix},rows={rows},tile={tile},{'plain' if plain else 'general'}>"


def default_plan(chain, blend, pix, h, w, options=None, keeps_state=False, per_frame_states=False):
    """The launcher's own choice for a warped render-loop launch, restated: the `warp=` string crtfx_last_plan must give.
    keeps_state: an unblended frame that also stores a float state (the first frame of a chain); per_frame_states: local_states."""
    o = options or {}
    if o.get("FORCE_GENERIC") or h * w * 12 >= 1 << 31:
        return "k_warp<gather>"
    rows = o.get("WARP_ROWS") or (2 if blend == "render" else 4)
    allowed = not o.get("NO_PLAIN_WARP")
    if blend == "none":
        plain = rows == 4 and allowed and not keeps_state and (w % 4 == 0 if pix == "u8" else w % 2 == 0)
    else:
        plain = rows == 2 and allowed and pix == "u8" and w % 4 == 0 and not per_frame_states
    return lean_plan(chain, blend, pix, rows, plain)


@dataclass(frozen=True)
class Row:
    name: str
    kernel: str                     # demangled instance name
    route: str                      # "loop" | "commit" | "api" | "preview"
    chain: str                      # "f32" | "f64"
    blend: str                      # "none" | "render" | "preview" | "float"
    pix: str                        # "u8" | "half"
    options: dict = field(default_factory=dict)
    plan: str = ""
    widths: str = "any"             # "any" | "w4" (W % 4 == 0) | "w2" (W even)
    extra: dict = field(default_factory=dict)      # route-specific: local_states, glitch, banded

    def fits(self, w):
        return self.widths == "any" or w % (4 if self.widths == "w4" else 2) == 0


def _rows():
    out = []
    for chain in ("f32", "f64"):
        prom = chain == "f64"
        for pix in ("u8", "half"):
            for r in (1, 2, 4):
                opts = {"WARP_ROWS": r, "NO_PLAIN_WARP": 1} if r == 4 else {"WARP_ROWS": r}
                out.append(Row(f"lean_{chain}_none_{pix}_rows{r}", lean_instance(prom, "none", pix, r), "loop", chain, "none", pix, opts,
                               lean_plan(chain, "none", pix, r)))
                out.append(Row(f"lean_{chain}_render_{pix}_rows{r}", lean_instance(prom, "render", pix, r), "loop", chain, "render", pix,
                               {"WARP_ROWS": r, "NO_PLAIN_WARP": 1}, lean_plan(chain, "render", pix, r)))
            # the branch-free builds, the planner's own choice on rows of whole dwords
            out.append(Row(f"plain_{chain}_none_{pix}", lean_instance(prom, "none", pix, 4, plain=True), "loop", chain, "none", pix, {},
                           lean_plan(chain, "none", pix, 4, True), "w4" if pix == "u8" else "w2"))
        out.append(Row(f"plain_{chain}_render_u8", lean_instance(prom, "render", "u8", 2, plain=True), "loop", chain, "render", "u8", {},
                       lean_plan(chain, "render", "u8", 2, True), "w4"))
        # the sharded render's per-frame states: every frame names its own state buffer, so the general build stores behind each frame
        out.append(Row(f"lean_{chain}_render_u8_local_states", lean_instance(prom, "render", "u8", 2), "loop", chain, "render", "u8", {},
                       lean_plan(chain, "render", "u8", 2), "any", {"local_states": True}))
        out.append(Row(f"lean_{chain}_render_half_local_states", lean_instance(prom, "render", "half", 2), "loop", chain, "render", "half", {},
                       lean_plan(chain, "render", "half", 2), "any", {"local_states": True}))
        # banded launches (y0 != 0) at rows 4 (the plain build on these widths) and rows 2
        out.append(Row(f"banded_{chain}_none_u8_rows4", lean_instance(prom, "none", "u8", 4, plain=True), "loop", chain, "none", "u8",
                       {"GROUP": 1, "BAND_MB": 1}, lean_plan(chain, "none", "u8", 4, True), "w4", {"banded": True}))
        out.append(Row(f"banded_{chain}_none_u8_rows4_general", lean_instance(prom, "none", "u8", 4), "loop", chain, "none", "u8",
                       {"GROUP": 1, "BAND_MB": 1, "NO_PLAIN_WARP": 1}, lean_plan(chain, "none", "u8", 4), "any", {"banded": True}))
        out.append(Row(f"banded_{chain}_none_u8_rows2", lean_instance(prom, "none", "u8", 2), "loop", chain, "none", "u8",
                       {"GROUP": 1, "BAND_MB": 1, "WARP_ROWS": 2}, lean_plan(chain, "none", "u8", 2), "any", {"banded": True}))
        out.append(Row(f"banded_{chain}_none_half_rows2", lean_instance(prom, "none", "half", 2), "loop", chain, "none", "half",
                       {"GROUP": 1, "BAND_MB": 1, "WARP_ROWS": 2}, lean_plan(chain, "none", "half", 2), "any", {"banded": True}))
        # warp 0 behind the Gaussian chain, a persistence chain of uint8 frames: the commit alone
        out.append(Row(f"commit_only_{chain}", lean_instance(prom, "render", "u8", 2, ident=True), "commit", chain, "render", "u8", {},
                       f"k_warp_lean<{chain},render,u8,rows=2,commit-only>"))
        # the general k_warp
        for pix in ("u8", "half"):
            out.append(Row(f"general_{chain}_api_{pix}", "crtfx::k_warp", "api", chain, "float", pix, {}, "k_warp<gather>"))
        out.append(Row(f"general_{chain}_api_glitch", "crtfx::k_warp", "api", chain, "float", "u8", {}, "k_warp<gather>", "any", {"glitch": True}))
        out.append(Row(f"general_{chain}_api_glitch_no_warp", "crtfx::k_warp", "api", chain, "float", "u8", {}, "k_warp<commit-only>", "any",
                       {"glitch": True, "no_warp": True}))
        out.append(Row(f"general_{chain}_preview", "crtfx::k_warp", "preview", chain, "preview", "u8", {}, "k_warp<gather>"))
        out.append(Row(f"general_{chain}_preview_glitch", "crtfx::k_warp", "preview", chain, "preview", "u8", {}, "k_warp<gather>", "any", {"glitch": True}))
        out.append(Row(f"general_{chain}_preview_glitch_no_warp", "crtfx::k_warp", "preview", chain, "preview", "u8", {}, "k_warp<commit-only>", "any",
                       {"glitch": True, "no_warp": True}))
        for blend in ("none", "render"):
            for pix in ("u8", "half"):
                out.append(Row(f"general_{chain}_loop_{blend}_{pix}", "crtfx::k_warp", "loop", chain, blend, pix, {"FORCE_GENERIC": 1}, "k_warp<gather>"))
        # a persistence chain of half frames with the warp off has no lean commit-only build: the general kernel's
        out.append(Row(f"general_{chain}_commit_only_half", "crtfx::k_warp", "commit", chain, "render", "half", {}, "k_warp<commit-only>"))
    return tuple(out)


ROWS = _rows()
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)


def covered_instances():
    return {r.kernel for r in ROWS}


def library_instances(resources):
    """The k_warp_lean<...> and k_warp kernels among tools/kernel_resources.resources' names."""
    return {k for k in resources if k.startswith("crtfx::k_warp_lean<") or k == "crtfx::k_warp"}
