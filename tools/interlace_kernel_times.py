"""Dev tool (GPU box): what the interlace stage (include/crtfx_interlace.h) costs per OUTPUT frame — uint8 / half x none / linear / complex
x vec path / general path; 480 x 720 and 1080 x 1920 — next to two yardsticks measured in the same run: a device-to-device copy of the same
traffic (the source bytes the stage must read + one frame written), and the untouched k_deint<linear,pix,both,vec> per SOURCE frame of its
own (one frame read, two written: the same three frames of traffic as a filtered weave).

    python tools/interlace_kernel_times.py run                  # HIP-event times per frame (launch gaps included) + the yardsticks + ratios

`run` launches, per size and kind, ROUNDS rounds of (vec, general, copy, deint), each WARM + RUNS batches timed with HIP events over the
RUNS back-to-back batches — a batch is FRAMES output frames, that is 2 * FRAMES source frames (FRAMES source frames for the deinterlacer) —
and prints the best round of each (the rounds alternate so that a neighbour's load on the machine hits all four) and the ratios to the copy.
The copy is torch's `copy_` of a buffer of half the traffic (it is read and written)."""
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [("480i", (480, 720)), ("1080i", (1080, 1920))]
PIXES = ["u8", "f16"]
FRAMES, WARM, RUNS, ROUNDS = 8, 3, 20, 3


def moved_bytes(size, pix, lowpass):
    """Of one output frame: under "none" every row is read from one of the two source frames (one frame's bytes); a filtered row reads its
    neighbours in its own frame, which the other parity's rows do not, so both source frames are read whole; one frame is written."""
    return size[0] * size[1] * 3 * (2 if pix == "f16" else 1) * ((1 if lowpass == "none" else 2) + 1)


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


def run():
    import torch
    import pythoncrt_amd as pc
    from pythoncrt_amd.interlace import LOWPASS
    dev = torch.device("cuda", torch.cuda.current_device())
    print(f"batches of {FRAMES} output frames ({2 * FRAMES} source frames), {WARM} warm-up + {RUNS} timed batches per figure, best of {ROUNDS} "
          "alternating rounds; us per OUTPUT frame from HIP events (launch gaps included); traffic = the source bytes read + one frame written; "
          f"the deinterlacer: batches of {FRAMES} source frames, us per SOURCE frame", flush=True)
    for (name, size), pix, lowpass in itertools.product(SIZES, PIXES, LOWPASS):
        mb = moved_bytes(size, pix, lowpass)
        if pix == "u8":
            frames = torch.randint(0, 256, (2 * FRAMES,) + size + (3,), dtype=torch.uint8, device=dev)
        else:
            frames = torch.randint(0, 1021, (2 * FRAMES,) + size + (3,), dtype=torch.int16, device=dev).to(torch.float16) / 4
        out = torch.empty((FRAMES,) + size + (3,), dtype=frames.dtype, device=dev)
        a = torch.empty((FRAMES, mb // 2), dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        plans = [pc.Interlace(dev, size, order="tff", lowpass=lowpass, dtype=frames.dtype, force_general=force) for force in (False, True)]
        deint = pc.Deinterlace(dev, size, method="linear", order="tff", fields="both", dtype=frames.dtype)
        best = {}
        for _ in range(ROUNDS):
            for key, fn in (("vec", lambda: plans[0].run(frames, out=out)), ("general", lambda: plans[1].run(frames, out=out)),
                            ("copy", lambda: b.copy_(a)), ("deint", lambda: deint.run(out, out=frames))):
                us = _timed(fn)
                best[key] = min(us, best.get(key, us))
        assert plans[0].plan()["interlace"].endswith("vec>") and plans[1].plan()["interlace"].endswith("general>")
        assert deint.plan()["deint"].endswith("both,vec>")
        for key, label in (("vec", plans[0].plan()["interlace"]), ("general", plans[1].plan()["interlace"]),
                           ("copy", "device-to-device copy of equal traffic"), ("deint", deint.plan()["deint"] + " (per source frame)")):
            mbk = moved_bytes(size, pix, "linear") if key == "deint" else mb       # the deinterlacer: one frame read, two written
            print(f"{name:6s} {label:50s} {best[key]:8.1f} us/frame {mbk / best[key] / 1e3:6.0f} GB/s of {mbk / 1e6:5.1f} MB"
                  + ("" if key in ("copy", "deint") else f"   {best[key] / best['copy']:5.2f} x the copy"), flush=True)
        for p in plans + [deint]:
            p.close()
        del frames, out, a, b
        torch.cuda.synchronize()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run()
        sys.exit(0)
    print(__doc__)
    sys.exit(2)
