"""The pointwise-chain kernel builds and how each one is reached: the table that drives tests/test_point_builds_gpu.py (every build held to
the oracle through the float32-storage model tests/warp_model.py on the GPU, bit for bit) and the CPU inventory in
tests/test_evidence_tools.py (every k_point* / k_half* instance in the library has a row).  No torch import here.

The launcher reaches 115 instances (crtfx.hip run_chain and "grouped path 2" of crtfx_process_batch):

  k_point_fused_seq  60   fast / fast+pixelate x {u8, half}; the one-knob builds +sat +luma +flicker -grain -vignette -triad -scanlines, +coarse,
                          +scan2d and +gradelut (u8); +grade and runtime x {u8, half}; each x blend {none, render}
  k_point_lean_seq   28   fast / fast+pixelate, +grade, runtime x {u8, half}; +gradelut and -bloom (u8); each x blend {none, render}
  k_point_lean        8   fast / fast+pixelate x {u8, half} x {none, render}: one frame per launch
  k_point_sel         4   {u8, half} x {one-round, two-round};  k_point_sel_seq the same four
  k_point<runtime>    1
  k_half / k_half_group  5 + 5   fast / fast+pixelate x {u8, half}, and the run-time gate word

A row names its instance(s) (template arguments as the demangler prints them: a second one where two kernels always launch together, the
half-resolution bloom source in front of the pointwise kernel), the route, the RenderSettings overrides on top of the reference CLI's
defaults, the pixel format, the blend, the DEBUG_OPTIONS, the shapes it is reachable on and the exact crtfx_last_plan `point=` (and
`half=`) strings it must produce.  Routes:

  loop      FramePipeline.run, several frames (crtfx_process_batch's grouped path): blend none = persistence 0, render = a persistence chain
            continued from a carried state, so that every frame of the batch blends and the whole batch is ONE launch;
  single    FramePipeline.run of ONE frame (crtfx_process_batch falls through to run_chain): the only way to k_point_lean — a float image
            (`api`) keeps a launch off the lean builds (`!k1.out_f32` in run_chain); blend render = a carried state, none = no state;
  api       apply_static_effects: one frame, its float image.

The gate words are computed from the sources (sf_words), never written as literals, and default_point_plan restates the launcher's choice."""
import os
import re
from dataclasses import dataclass, field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PIX = {"u8": 0, "half": 1}
BLEND = {"none": 0, "render": 1}

# process_video's effect keywords with the reference CLI's defaults (pythoncrt_amd.pipeline.RenderSettings, restated: no torch import here;
# tests/test_point_model.py holds the two together)
DEFAULTS = dict(scanline_strength=0.6, triad_strength=0.35, triad_gamma=2.2, triad_preserve_luma=False, triad_softness=0.5, aberration_px=1,
                bloom_sigma=1.2, bloom_strength=0.25, bloom_threshold=0.0, noise_strength=1.5, vignette_strength=0.25, persistence=0.2,
                scanline_speed_px_s=30.0, scanline_period_px=2.0, fast_bloom=True, pixel_size=2, brightness=0.0, contrast=1.0, gamma=1.0,
                saturation=1.0, temperature=0.0, flicker_strength=0.0, flicker_hz=0.0, grain_size=1, scanline_angle=0.0,
                scanline_thickness=1.0, warp_strength=0.0, glitch_amp_px=0, glitch_height_frac=0.0)


# ---- the gate words, from the sources ----------------------------------------------------------------------------------------------
def _eval(expr, names):
    """A constant expression of the headers: names, `1u << n`, hex / decimal literals, `|`, `&`, `~`, parentheses, (uint32_t) casts."""
    e = expr.replace("(uint32_t)", "")
    e = re.sub(r"\b(0x[0-9A-Fa-f]+|\d+)u\b", r"\1", e)
    e = re.sub(r"\b[A-Z][A-Z0-9_]+\b", lambda m: str(names[m.group(0)]), e)
    assert re.fullmatch(r"[0-9xA-Fa-f\s|&~()<]+", e), expr
    return eval(e, {"__builtins__": {}}) & 0xFFFFFFFF      # noqa: S307  (digits and operators only, checked above)


_WORDS = None


def sf_words():
    """Every constant the launcher's choice is made of, as the sources define it: CRTFX_F_* from include/crtfx.h; KF_*, SF_FULL_GATES, SF_FAST,
    SF_FAST_PIX, SF_LEAN_RT and GRADE_RT_MASK from crtfx_common.hip.h; SF_RUNTIME from crtfx_phosphor.hip.h; SF_NOBLOOM[_PIX] and the
    one-knob sets (CRTFX_KNOB_SETS) from crtfx.hip."""
    global _WORDS
    if _WORDS is not None:
        return _WORDS
    src = lambda *p: open(os.path.join(ROOT, *p)).read()      # noqa: E731
    w = {m.group(1): 1 << int(m.group(2)) for m in re.finditer(r"#define\s+(CRTFX_F_[A-Z_]+)\s+\(1u\s*<<\s*(\d+)\)", src("include", "crtfx.h"))}
    common = src("pythoncrt_amd", "csrc", "crtfx_common.hip.h")
    for name in ("KF_VIG_UNIT", "SF_FULL_GATES", "SF_FAST", "SF_FAST_PIX", "SF_LEAN_RT", "KF_GRADE_RT", "KF_GRADE_LUT", "KF_COARSE", "KF_SCANPLANE",
                 "GRADE_RT_MASK"):
        w[name] = _eval(re.search(rf"constexpr uint32_t {name} = ([^;]+);", common).group(1), w)
    w["SF_RUNTIME"] = _eval(re.search(r"constexpr uint32_t SF_RUNTIME = ([^;]+);", src("pythoncrt_amd", "csrc", "crtfx_phosphor.hip.h")).group(1), w)
    host = src("pythoncrt_amd", "csrc", "crtfx.hip")
    m = re.search(r"constexpr uint32_t SF_NOBLOOM = ([^,;]+), SF_NOBLOOM_PIX = ([^;]+);", host)
    w["SF_NOBLOOM"] = _eval(m.group(1), w)
    w["SF_NOBLOOM_PIX"] = _eval(m.group(2), w)
    knobs = re.search(r"#define CRTFX_KNOB_SETS\(X\)(.*?)\n#define CRTFX_KNOB_NAME", host, re.S).group(1).replace("\\\n", " ")
    w["KNOBS"] = {}
    for op, name in re.findall(r'X\(\s*([|&][^"]+?),\s*"([^"]+)"\)', knobs):      # X(| CRTFX_F_SATURATION, "+sat") ...
        w["KNOBS"][name] = (_eval("SF_FAST " + op, w), _eval("SF_FAST_PIX " + op, w))
    _WORDS = w
    return w


def gate_names():
    """{the gate name of a plan string: (word without pixelate, word with)} for the lean / fused families."""
    w = sf_words()
    out = {"": (w["SF_FAST"], w["SF_FAST_PIX"]), "-bloom": (w["SF_NOBLOOM"], w["SF_NOBLOOM_PIX"])}
    out.update(w["KNOBS"])
    for name, bit in (("+coarse", "KF_COARSE"), ("+scan2d", "KF_SCANPLANE"), ("+gradelut", "KF_GRADE_LUT"), ("+grade", "KF_GRADE_RT")):
        out[name] = (w["SF_FAST"] | w[bit], w["SF_FAST_PIX"] | w[bit])
    return out


def plan_instance(plan):
    """The demangled instance (tools/kernel_resources.resources) behind one crtfx_last_plan `point=` / `half=` string."""
    w = sf_words()
    m = re.fullmatch(r"(k_[a-z_]+)<(.*)>", plan)
    fam, args = m.group(1), m.group(2).split(",")
    if fam == "k_point":
        assert args == ["runtime"]
        return f"crtfx::k_point<{w['SF_RUNTIME']}u>"
    if fam in ("k_point_sel", "k_point_sel_seq"):
        return f"crtfx::{fam}<{PIX[args[0]]}, {'true' if args[1] == 'one-round' else 'false'}>"
    if fam in ("k_half", "k_half_group"):
        if args == ["runtime", "any"]:
            return f"crtfx::{fam}<{w['SF_RUNTIME']}u, 0>"
        return f"crtfx::{fam}<{w['SF_FAST_PIX'] if args[0] == 'fast+pixelate' else w['SF_FAST']}u, {PIX[args[1]]}>"
    assert fam in ("k_point_lean", "k_point_lean_seq", "k_point_fused_seq"), plan
    gate, pix, blend = args
    if gate == "runtime":
        word = w["SF_LEAN_RT"]
    else:
        m = re.fullmatch(r"fast(\+pixelate)?(.*)", gate)
        word = gate_names()[m.group(2)][1 if m.group(1) else 0]
    return f"crtfx::{fam}<{word}u, {PIX[pix]}, {BLEND[blend]}>"


# ---- the launcher's choice, restated --------------------------------------------------------------------------------------------------
def gate_flags(settings, pix):
    """(the gate word crtfx_set_params keeps — Engine.set_params' CRTFX_F_* bits plus KF_VIG_UNIT —, whether a grade table is uploaded)."""
    w = sf_words()
    s = dict(DEFAULTS, **settings)
    fl = 0
    if s["saturation"] != 1.0:
        fl |= w["CRTFX_F_SATURATION"]
    if s["temperature"] != 0.0:
        fl |= w["CRTFX_F_TEMPERATURE"]
    if s["brightness"] != 0.0 or s["contrast"] != 1.0:
        fl |= w["CRTFX_F_BRIGHTCON"]
    if s["gamma"] != 1.0 and s["gamma"] > 0.0:
        fl |= w["CRTFX_F_GAMMA"]
    glut = pix == "u8" and not fl & w["CRTFX_F_SATURATION"] and bool(fl & (w["CRTFX_F_TEMPERATURE"] | w["CRTFX_F_BRIGHTCON"] | w["CRTFX_F_GAMMA"]))
    if s["pixel_size"] > 1:
        fl |= w["CRTFX_F_PIXELATE"]
    if s["bloom_strength"] > 0.0 and (s["bloom_sigma"] > 0.0 or s["fast_bloom"]):
        fl |= w["CRTFX_F_BLOOM"]
        if s["fast_bloom"]:
            fl |= w["CRTFX_F_BLOOM_FAST"]
        if s["bloom_threshold"] > 0.0:
            fl |= w["CRTFX_F_BLOOM_THR"]
    if s["triad_strength"] > 0.0:
        fl |= w["CRTFX_F_TRIAD"]
        if s["triad_preserve_luma"] or not abs(float(s["triad_gamma"]) - 1.0) < 1e-3:      # tables.triad_uses_lut (triad_gamma > 0)
            fl |= w["CRTFX_F_TRIAD_LUT"]
            if s["triad_preserve_luma"]:
                fl |= w["CRTFX_F_TRIAD_LUMA"]
    if s["scanline_strength"] > 0.0:
        fl |= w["CRTFX_F_SCANLINES"]
    if s["vignette_strength"] > 0.0:
        fl |= w["CRTFX_F_VIGNETTE"]
        if 0.0 <= s["vignette_strength"] <= 1.0:
            fl |= w["KF_VIG_UNIT"]
    if s["flicker_strength"] > 0.0 and s["flicker_hz"] > 0.0:
        fl |= w["CRTFX_F_FLICKER"]
    if s["noise_strength"] > 0.0:
        fl |= w["CRTFX_F_NOISE"]
    if s["warp_strength"] != 0.0:
        fl |= w["CRTFX_F_WARP"]
    return fl, glut


def _sf_name(word):
    w = sf_words()
    return "fast" if word == w["SF_FAST"] else "fast+pixelate" if word == w["SF_FAST_PIX"] else "runtime" if word == w["SF_RUNTIME"] else "full"


def default_point_plan(settings, pix, h, w_, options=None, blend="none", frames=2, float_out=False, injected_planes=False):
    """The launcher's own choice for the pointwise chain, restated: {"point": ..., "half": ...} as crtfx_last_plan must give them ("half"
    only where a k_half* launch belongs to it).  `frames`: the frames of the launch group (every frame with the same blend); 1 = the
    one-frame path (run_chain).  float_out: apply_static_effects' float image.  injected_planes: grain planes handed in per frame."""
    w = sf_words()
    o = options or {}
    s = dict(DEFAULTS, **settings)
    fl, glut = gate_flags(settings, pix)
    assert not fl & w["CRTFX_F_WARP"], "the pointwise rows run with the warp off"
    gates = fl
    bloom = bool(fl & w["CRTFX_F_BLOOM"])
    fastb = bloom and bool(fl & w["CRTFX_F_BLOOM_FAST"])
    assert fastb or not bloom, "a Gaussian bloom is the phosphor kernels' chain, not the pointwise one"
    pixelate = bool(fl & w["CRTFX_F_PIXELATE"])
    fast_words = (w["SF_FAST"], w["SF_FAST_PIX"])
    force_generic, force_rt = bool(o.get("FORCE_GENERIC")), bool(o.get("FORCE_RUNTIME_FLAGS"))
    scan_plane = bool(fl & w["CRTFX_F_SCANLINES"]) and not (s["scanline_angle"] == 0.0 and s["scanline_thickness"] == 1.0)
    coarse = bool(fl & w["CRTFX_F_NOISE"]) and s["grain_size"] > 1
    rounds = "one-round" if (not pixelate and not fastb) else "two-round"
    out = {}
    if frames >= 2 and not force_generic:
        # ---- grouped path 2 of crtfx_process_batch
        waves = o.get("POINT_TILES") or 8
        exact_2x = max(1, w_ // 2) * 2 == w_ and max(1, h // 2) * 2 == h          # else the host hands in the fbd_* tap tables (kp.dx_ofs)
        can_fuse = fastb and not o.get("NO_FUSED_HALF") and exact_2x and 4 <= waves <= 8
        thr = bool(gates & w["CRTFX_F_BLOOM_THR"])
        gates_nt = gates & ~w["CRTFX_F_BLOOM_THR"]
        coarse_knob = coarse and can_fuse and not force_rt and pix == "u8" and gates_nt in fast_words
        lean = not force_rt and (not coarse or coarse_knob) and not injected_planes
        scan_ok = can_fuse and not coarse and pix == "u8" and gates_nt in fast_words
        folded_gates = gates_nt in fast_words and not coarse
        knob = "+coarse" if coarse_knob else None
        if not folded_gates and not coarse and pix == "u8":
            for name, words in w["KNOBS"].items():
                if gates_nt in words:
                    knob = name
        nobloom = not folded_gates and pix == "u8" and gates_nt in (w["SF_NOBLOOM"], w["SF_NOBLOOM_PIX"])
        grade_any = not folded_gates and (gates & ~w["GRADE_RT_MASK"]) in fast_words
        per_channel = w["CRTFX_F_TEMPERATURE"] | w["CRTFX_F_BRIGHTCON"] | w["CRTFX_F_GAMMA"]
        grade_lut = grade_any and pix == "u8" and glut and (gates_nt & w["GRADE_RT_MASK"] & ~per_channel) == 0
        grade_rt = grade_any and not grade_lut
        scan_knob = scan_plane and scan_ok and lean
        if scan_plane and not scan_knob:
            lean = False
        fused = lean and can_fuse
        knob_build = fused and (knob is not None or scan_knob)
        pre = "fast+pixelate" if pixelate else "fast"
        if folded_gates and not scan_knob:
            gname = _sf_name(gates_nt)
        elif knob_build:
            gname = pre + ("+scan2d" if scan_knob else knob)
        elif nobloom:
            gname = pre + "-bloom"
        elif grade_lut:
            gname = pre + "+gradelut"
        elif grade_rt:
            gname = pre + "+grade"
        else:
            gname = "runtime"
        if fastb and not fused:
            fold = lean and folded_gates and not thr
            out["half"] = f"k_half_group<{_sf_name(gates) if fold else 'runtime'},{pix if fold else 'any'}>"
        if lean:
            out["point"] = f"{'k_point_fused_seq' if fused else 'k_point_lean_seq'}<{gname},{pix},{blend}>"
        else:
            out["point"] = f"k_point_sel_seq<{pix},{rounds}>"
        return out
    # ---- run_chain: one frame
    if fastb:
        fold = not force_generic and not force_rt and gates in fast_words
        out["half"] = f"k_half<{_sf_name(gates) if fold else 'runtime'},{pix if fold else 'any'}>"
    lean = (not force_generic and not force_rt and gates in fast_words and not scan_plane and not injected_planes and s["grain_size"] <= 1
            and not float_out)
    if lean:
        out["point"] = f"k_point_lean<{_sf_name(gates)},{pix},{blend}>"
    elif not force_generic:
        out["point"] = f"k_point_sel<{pix},{rounds}>"
    else:
        out["point"] = "k_point<runtime>"
    return out


# ---- the rows ---------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Row:
    name: str
    kernels: tuple                  # demangled instance names: the pointwise kernel, then the k_half* launch in front of it (if any)
    route: str                      # "loop" | "single" | "api"
    settings: dict                  # RenderSettings overrides on top of the CLI defaults (persistence is the blend's: see `blend`)
    pix: str                        # "u8" | "half"
    blend: str                      # "none" | "render"
    options: dict = field(default_factory=dict)
    shapes: str = "any"             # "even" (the fused kernel: exact 2x decimation) | "any"
    point: str = ""                 # crtfx_last_plan point=
    half: str = ""                  # crtfx_last_plan half= ("" = no k_half* launch)
    gamma_family: str = ""          # the grade family this row's extra gamma case stands for ("" = none)
    note: str = ""

    def fits(self, h, w):
        return self.shapes == "any" or (h % 2 == 0 and w % 2 == 0)


# one setting per gate name (on top of the defaults); pixelate is the row's own axis
KNOB_SETTINGS = {
    "+sat": dict(saturation=1.2), "+luma": dict(triad_preserve_luma=True), "+flicker": dict(flicker_strength=0.4, flicker_hz=9.0),
    "-grain": dict(noise_strength=0.0), "-vignette": dict(vignette_strength=0.0), "-triad": dict(triad_strength=0.0),
    "-scanlines": dict(scanline_strength=0.0), "+coarse": dict(grain_size=2), "+scan2d": dict(scanline_angle=10.0, scanline_thickness=2.0),
    "+gradelut": dict(brightness=0.05, contrast=1.1, temperature=0.3), "-bloom": dict(bloom_strength=0.0),
}
# the arithmetic grade (KF_GRADE_RT): what the table cannot express — uint8 frames need a second gate next to the saturation (one knob alone has
# a folded build), half frames take every grade here
GRADE_RT_SETTINGS = {"u8": dict(saturation=1.3, temperature=-0.4, brightness=0.04, contrast=1.2, bloom_threshold=0.3),
                     "half": dict(brightness=0.05, contrast=1.1, triad_preserve_luma=True)}
# the gate word at run time (SF_LEAN_RT): two stages off — (a) no vignette: the chain stays float32; (b) promoted, with a grade and a flicker
RUNTIME_SETTINGS = {"a": dict(vignette_strength=0.0, noise_strength=0.0), "b": dict(triad_strength=0.0, scanline_strength=0.0, contrast=1.15,
                                                                                   flicker_strength=0.3, flicker_hz=7.0)}


def _row(name, route, settings, pix, blend, options=None, shapes="any", frames=4, float_out=False, **kw):
    """A row whose plan strings are the restated launcher's for the smallest shape of its class, and whose instances are those strings'."""
    h, w = (34, 66) if shapes == "even" else (37, 131)
    plan = default_point_plan(settings, pix, h, w, options, blend, frames, float_out)
    kernels = (plan_instance(plan["point"]),) + ((plan_instance(plan["half"]),) if "half" in plan else ())
    return Row(name, kernels, route, dict(settings), pix, blend, dict(options or {}), shapes, plan["point"], plan.get("half", ""), **kw)


def _rows():
    out = []
    two = {"NO_FUSED_HALF": 1}
    for blend in ("none", "render"):
        for pixelate in (False, True):
            # the pixelate rows: the default cell of 2 (the fused prologue fetches a cell once) without a blend, 3 (a partial last cell on every shape) with one
            ps = dict(pixel_size=(2 if blend == "none" else 3) if pixelate else 1)
            tag = ("pix_" if pixelate else "") + blend
            for pix in ("u8", "half"):
                # the reference CLI's default gate set: fused, and on k_half_group + k_point_lean_seq
                out.append(_row(f"fused_fast_{pix}_{tag}", "loop", ps, pix, blend, {}, "even"))
                out.append(_row(f"lean_fast_{pix}_{tag}", "loop", ps, pix, blend, two))
                g = dict(ps, **GRADE_RT_SETTINGS[pix])
                fam = f"+grade {pix}" if (blend == "render" and not pixelate) else ""
                out.append(_row(f"fused_grade_{pix}_{tag}", "loop", g, pix, blend, {}, "even", gamma_family=fam))
                out.append(_row(f"lean_grade_{pix}_{tag}", "loop", g, pix, blend, two))
            for name, st in KNOB_SETTINGS.items():
                if name == "-bloom":
                    out.append(_row(f"lean_nobloom_u8_{tag}", "loop", dict(ps, **st), "u8", blend))
                    continue
                fam = "+gradelut" if (name == "+gradelut" and blend == "render" and not pixelate) else ""
                out.append(_row(f"fused_{name[1:]}_u8_{tag}", "loop", dict(ps, **st), "u8", blend, {}, "even", gamma_family=fam))
                if name == "+gradelut":
                    out.append(_row(f"lean_gradelut_u8_{tag}", "loop", dict(ps, **st), "u8", blend, two))
        # the run-time gate word: both chain dtypes on every instance
        for pix in ("u8", "half"):
            for k, st in RUNTIME_SETTINGS.items():
                st = dict(st, pixel_size=1 if k == "a" else 2)
                fam = "runtime" if (blend == "render" and pix == "u8" and k == "b") else ""
                out.append(_row(f"fused_runtime_{k}_{pix}_{blend}", "loop", st, pix, blend, {}, "even", gamma_family=fam))
                out.append(_row(f"lean_runtime_{k}_{pix}_{blend}", "loop", st, pix, blend, two))
    # the general sequence kernel: the gate word forced to run time (k_half_group<runtime> in front of the two-round build) ...
    for pix in ("u8", "half"):
        out.append(_row(f"sel_seq_two_round_{pix}", "loop", {}, pix, "render", {"FORCE_RUNTIME_FLAGS": 1}))
        out.append(_row(f"sel_seq_one_round_{pix}", "loop", dict(pixel_size=1, bloom_strength=0.0), pix, "none", {"FORCE_RUNTIME_FLAGS": 1}))
    # ... and where the planner itself lands on it: coarse grain on half frames (the lean coarse build is uint8 only)
    out.append(_row("sel_seq_coarse_half", "loop", dict(grain_size=2), "half", "render"))
    # one frame per launch: k_half in front of k_point_lean
    for pix in ("u8", "half"):
        for pixelate in (False, True):
            for blend in ("none", "render"):
                out.append(_row(f"lean1_{pix}_{'pix_' if pixelate else ''}{blend}", "single", dict(pixel_size=3 if pixelate else 1), pix, blend, frames=1))
    # the float image: k_half in front of k_point_sel (two rounds: a load address depends on a load), one round without bloom and pixelate
    for pix in ("u8", "half"):
        out.append(_row(f"sel_two_round_{pix}", "api", dict(pixel_size=1 if pix == "u8" else 3), pix, "none", frames=1, float_out=True))
        out.append(_row(f"sel_one_round_{pix}", "api", dict(pixel_size=1, bloom_strength=0.0, saturation=1.25), pix, "none", frames=1, float_out=True))
    out.append(_row("sel_threshold_u8", "api", dict(bloom_threshold=0.3), "u8", "none", frames=1, float_out=True))      # k_half<runtime>
    out.append(_row("generic_u8", "api", {}, "u8", "none", {"FORCE_GENERIC": 1}, frames=1, float_out=True))
    out.append(_row("generic_half", "api", dict(pixel_size=1, contrast=1.1), "half", "none", {"FORCE_GENERIC": 1}, frames=1, float_out=True))
    return tuple(out)


ROWS = _rows()
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)

# the shapes of tests/test_point_builds_gpu.py: the smallest at which a 64-pixel-wide tile of 8 waves x CRTFX_POINT_ROWS = 16 rows can go wrong
SHAPES = {"tiny": (2, 2), "ragged": (34, 66), "strips": (50, 198), "odd": (37, 131)}


def row_shapes(row):
    return [k for k, (h, w) in SHAPES.items() if row.fits(h, w) and (row.shapes == "any" or k != "odd")]


def covered_instances():
    return {k for r in ROWS for k in r.kernels}


def library_instances(resources):
    """The k_point* / k_half* kernels among tools/kernel_resources.resources' names."""
    return {k for k in resources if re.match(r"crtfx::k_(point|half)[a-z_]*<", k)}
