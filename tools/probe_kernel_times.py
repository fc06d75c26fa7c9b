"""Dev tool (GPU box): what the source probe (include/crtfx_probe.h) costs per frame — uint8 / half x vec path / general path; 480 x 720
and 1080 x 1920; three contents — next to two yardsticks measured in the same run: a device-to-device copy that reads the same bytes, and
the untouched k_adeint<...,first,vec> of include/crtfx_adeint.h, which reads the same frames and writes them too.

    python tools/probe_kernel_times.py run                      # HIP-event times per frame (launch gaps included) + the yardsticks + ratios

`run` launches, per size, kind and content, ROUNDS rounds of (vec, general, adeint vec, copy), each WARM + RUNS batches of FRAMES frames
timed with HIP events over the RUNS back-to-back batches, and prints the best round of each (the rounds alternate so that a neighbour's
load on the machine hits all four) and the ratios.  Every frame has a previous frame (frame 0 the caller's).  The contents: "random" —
uniform noise, every lane another bin; "constant" — one value, every lane of every wave the same bin, the atomics' worst case; "boxed" —
black bars above and below a picture of noise in which a block moves.  The probe's time includes the kernel that initialises the records.
The copy is torch's `copy_` of a buffer of the frames' size (read once, written once: twice the probe's traffic to memory)."""
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [("480", (480, 720)), ("1080", (1080, 1920))]
PIXES = ["u8", "f16"]
CONTENTS = ["random", "constant", "boxed"]
FRAMES, WARM, RUNS, ROUNDS = 8, 3, 20, 3


def _timed(fn):
    import torch
    for _ in range(WARM):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(RUNS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (RUNS * FRAMES)


def _content(kind, size, dev):
    """FRAMES + 1 uint8 frames."""
    import torch
    h, w = size
    if kind == "constant":
        return torch.full((FRAMES + 1, h, w, 3), 128, dtype=torch.uint8, device=dev)
    frames = torch.randint(0, 256, (FRAMES + 1, h, w, 3), dtype=torch.uint8, device=dev)
    if kind == "boxed":
        frames[1:] = frames[0]
        for i in range(FRAMES + 1):
            frames[i, h // 3:h // 2, 16 * i:16 * i + w // 4] = 200
        frames[:, :h // 8] = 0
        frames[:, h - h // 8:] = 0
    return frames


def run():
    import torch
    import pythoncrt_amd as pc
    dev = torch.device("cuda", torch.cuda.current_device())
    print(f"batches of {FRAMES} frames, {WARM} warm-up + {RUNS} timed batches per figure, best of {ROUNDS} alternating rounds; us per frame from HIP "
          "events (launch gaps included)", flush=True)
    for (name, size), pix, kind in itertools.product(SIZES, PIXES, CONTENTS):
        frames = _content(kind, size, dev)
        if pix == "f16":
            frames = frames.to(torch.float16)
        prev, frames = frames[0], frames[1:]
        nbytes = frames[0].numel() * frames.element_size()
        probes = [pc.Probe(dev, size, dtype=frames.dtype, force_general=force) for force in (False, True)]
        adeint = pc.AdaptiveDeinterlace(dev, size, order="tff", fields="first", dtype=frames.dtype)
        rec = torch.empty((FRAMES, probes[0].words), dtype=torch.uint32, device=dev)
        out = torch.empty_like(frames)
        a = frames.clone()
        best = {}
        for _ in range(ROUNDS):
            for key, fn in (("vec", lambda: probes[0].run(frames, prev=prev, out=rec)), ("general", lambda: probes[1].run(frames, prev=prev, out=rec)),
                            ("adeint vec", lambda: adeint.run(frames, out=out, prev=prev)), ("copy", lambda: out.copy_(a))):
                us = _timed(fn)
                best[key] = min(us, best.get(key, us))
        assert probes[0].plan()["probe"].endswith("vec>") and probes[1].plan()["probe"].endswith("general>") and adeint.plan()["adeint"].endswith("first,vec>")
        for key, label in (("vec", probes[0].plan()["probe"]), ("general", probes[1].plan()["probe"]), ("adeint vec", adeint.plan()["adeint"]),
                           ("copy", "device-to-device copy of the frames")):
            ratios = "" if key == "copy" else f"   {best[key] / best['copy']:5.2f} x the copy"
            if key in ("vec", "general"):
                ratios += f"   {best[key] / best['adeint vec']:5.2f} x adeint vec"
            print(f"{name:5s} {pix:3s} {kind:8s} {label:38s} {best[key]:8.1f} us/frame {nbytes / best[key] / 1e3:6.0f} GB/s of {nbytes / 1e6:5.1f} MB read" + ratios, flush=True)
        print(f"{name:5s} {pix:3s} {kind:8s} vec / general = {best['vec'] / best['general']:.2f}", flush=True)
        for p in probes + [adeint]:
            p.close()
        del frames, prev, out, a, rec
        torch.cuda.synchronize()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run()
        sys.exit(0)
    print(__doc__)
    sys.exit(2)
