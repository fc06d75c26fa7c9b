"""The per-radius k_phosphor builds and how each one is reached: the table that drives tests/test_radius_builds_gpu.py (every build held to
the oracle on the GPU) and the CPU inventory in tests/test_evidence_tools.py (every build in the library has a row).  No torch import here.

A row names its kernel family, the gate word of the template (`full`, `full+pixelate`, `runtime`; None for the families that fold the
full-chain gates into the kernel itself), the pixel format, the radii it covers, the settings and DEBUG_OPTIONS that select it, the route
(`api`: apply_static_effects, one frame, its float image; `loop`: FramePipeline.run, a persistence chain with no warp, so a pre-warp image
is parked and frame 0's per-frame state is that image) and the crtfx_last_plan phosphor string it must produce."""
import os
import re
from dataclasses import dataclass, field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TW, NB = 64, 8                      # strip width and rows per block of the register-window kernels (crtfx_common.hip.h)
RR_RADII = tuple(range(1, 31))      # one crtfx_rr.hip build per radius (pythoncrt_amd/_lib.py RR_RADII)
CT_RADII = tuple(range(1, 16))      # k_phosphor_ct: CT_MAX_RADIUS = CT_HALF_MAX_RADIUS = 15
GENERIC_RADII = tuple(range(1, 65))  # k_phosphor<-1>: GENERIC_MAX_RADIUS = 64

# the full-chain gate set (BASELINE configs 2-5): Gaussian bloom, softened triad through its LUTs, row scanlines, analytic vignette, grain
FULL = dict(scanline_strength=0.6, triad=(0.35, 0.5), vignette=0.25, bloom_strength=0.25, bloom_threshold=0.0, noise_strength=1.5,
            pixel_size=1)


@dataclass(frozen=True)
class Build:
    name: str
    family: str                     # k_phosphor_ct / k_phosphor_cc / k_phosphor_rr / k_phosphor
    gates: str                      # "full" | "full+pixelate" | "runtime" (k_phosphor_rr's SF word); "" for the other families
    pix: str                        # "u8" | "half"
    radii: tuple
    route: str                      # "api" | "loop"
    options: dict = field(default_factory=dict)
    settings: dict = field(default_factory=dict)
    plan: str = ""                  # crtfx_last_plan phosphor, "{R}" = the radius

    def plan_for(self, R):
        return self.plan.format(R=R)

    def options_for(self, R):
        opts = dict(self.options)
        if self.family == "k_phosphor" and R > 30:
            opts["SPLIT_FROM"] = 65        # radii 31 .. 64 would take the split path by default
        return opts


BUILDS = (
    Build("ct_u8", "k_phosphor_ct", "", "u8", CT_RADII, "loop", {}, {}, "k_phosphor_ct<{R},u8>"),
    Build("cc_u8", "k_phosphor_cc", "", "u8", RR_RADII, "loop", {"FORCE_CC": 1, "NO_CT": 1}, {}, "k_phosphor_cc<{R},u8>"),
    Build("cc_u8_default", "k_phosphor_cc", "", "u8", tuple(range(16, 31)), "loop", {}, {}, "k_phosphor_cc<{R},u8>"),     # the planner's own choice
    Build("rr_full_u8", "k_phosphor_rr", "full", "u8", RR_RADII, "api", {"NO_CC": 1}, {}, "k_phosphor_rr<{R},full,u8>"),
    Build("rr_pix_u8", "k_phosphor_rr", "full+pixelate", "u8", RR_RADII, "api", {}, {"pixel_size": (2, 3)}, "k_phosphor_rr<{R},full+pixelate,u8>"),
    Build("rr_rt_u8", "k_phosphor_rr", "runtime", "u8", RR_RADII, "api", {"FORCE_RUNTIME_FLAGS": 1}, {"bloom_threshold": 0.2},
          "k_phosphor_rr<{R},runtime,u8>"),
    Build("ct_half", "k_phosphor_ct", "", "half", CT_RADII, "loop", {}, {}, "k_phosphor_ct<{R},half>"),
    Build("rr_full_half", "k_phosphor_rr", "full", "half", RR_RADII, "api", {"NO_CT": 1}, {}, "k_phosphor_rr<{R},full,half>"),
    Build("rr_rt_half", "k_phosphor_rr", "runtime", "half", RR_RADII, "api", {"FORCE_RUNTIME_FLAGS": 1}, {"bloom_threshold": 0.2},
          "k_phosphor_rr<{R},runtime,half>"),
    Build("generic", "k_phosphor", "", "", GENERIC_RADII, "api", {"FORCE_GENERIC": 1}, {}, "k_phosphor<-1>"),
)
BY_NAME = {b.name: b for b in BUILDS}


def sf_words():
    """{"full": SF_FULL, "full+pixelate": SF_FULL | CRTFX_F_PIXELATE, "runtime": SF_RUNTIME} as the sources define them: CRTFX_F_* from
    include/crtfx.h, KF_VIG_UNIT and SF_FULL_GATES from crtfx_common.hip.h, SF_RUNTIME from crtfx_phosphor.hip.h."""
    hdr = open(os.path.join(ROOT, "include", "crtfx.h")).read()
    consts = {m.group(1): 1 << int(m.group(2)) for m in re.finditer(r"#define\s+(CRTFX_F_[A-Z_]+)\s+\(1u\s*<<\s*(\d+)\)", hdr)}
    common = open(os.path.join(ROOT, "pythoncrt_amd", "csrc", "crtfx_common.hip.h")).read()
    m = re.search(r"constexpr uint32_t KF_VIG_UNIT = 1u << (\d+);", common)
    consts["KF_VIG_UNIT"] = 1 << int(m.group(1))
    m = re.search(r"constexpr uint32_t SF_FULL_GATES = ([^;]+);", common)
    full = 0
    for term in m.group(1).split("|"):
        full |= consts[term.strip()]
    phos = open(os.path.join(ROOT, "pythoncrt_amd", "csrc", "crtfx_phosphor.hip.h")).read()
    assert re.search(r"constexpr uint32_t SF_FULL = SF_FULL_GATES;", phos), "SF_FULL is no longer SF_FULL_GATES"
    rt = int(re.search(r"constexpr uint32_t SF_RUNTIME = (0x[0-9A-Fa-f]+)u;", phos).group(1), 16)
    return {"full": full, "full+pixelate": full | consts["CRTFX_F_PIXELATE"], "runtime": rt}


def instances(build, words=None):
    """The demangled kernel names (tools/kernel_resources.resources) that `build` covers."""
    pix = {"u8": 0, "half": 1}
    if build.family == "k_phosphor":
        return {"crtfx::k_phosphor<-1>"}
    if build.family == "k_phosphor_rr":
        words = words or sf_words()
        return {f"crtfx::k_phosphor_rr<{r}, {words[build.gates]}u, {pix[build.pix]}>" for r in build.radii}
    return {f"crtfx::{build.family}<{r}, {pix[build.pix]}>" for r in build.radii}


def covered_instances():
    words = sf_words()
    out = set()
    for b in BUILDS:
        out |= instances(b, words)
    return out
