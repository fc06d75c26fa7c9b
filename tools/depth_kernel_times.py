"""Dev tool (GPU box): what the depth stage (include/crtfx_depth.h) costs per frame — widen, narrow without dither, narrow with the ordered
dither; vec path and general path; 1080p and 4K — next to a yardstick measured in the same run: a device-to-device copy of the same
traffic (a frame's uint8 bytes + its half bytes: one side is read, the other written).

    python tools/depth_kernel_times.py run                      # HIP-event times per frame (launch gaps included) + the copies + ratios
    rocprofv3 --kernel-trace --stats -d DIR -o depth --output-format csv -- python tools/depth_kernel_times.py run
    python tools/depth_kernel_times.py report DIR               # kernel time per frame from the trace

`run` launches, per size and kind, ROUNDS rounds of (vec, general, copy), each WARM + RUNS batches of FRAMES frames timed with HIP events
over the RUNS back-to-back batches, and prints the best round of each (the rounds alternate so that a neighbour's load on the machine hits
all three) and the ratios to the copy.  The copy is torch's `copy_` of a buffer of half the traffic (it is read and written).
`report` walks the trace's k_widen / k_narrow dispatches in that order, drops each WARM part, and prints mean kernel time per frame."""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [("1080p", (1080, 1920)), ("4K", (2160, 3840))]
KINDS = [("widen", "none"), ("narrow", "none"), ("narrow", "ordered")]
FRAMES, WARM, RUNS, ROUNDS = 8, 3, 20, 3


def moved_bytes(size):
    return size[0] * size[1] * 3 * (1 + 2)


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
    dev = torch.device("cuda", torch.cuda.current_device())
    print(f"batches of {FRAMES} frames, {WARM} warm-up + {RUNS} timed batches per figure, best of {ROUNDS} alternating rounds; us per frame from HIP "
          "events (launch gaps included); traffic = uint8 frame bytes + half frame bytes", flush=True)
    for name, size in SIZES:
        mb = moved_bytes(size)
        for kind, dither in KINDS:
            u8 = torch.randint(0, 256, (FRAMES,) + size + (3,), dtype=torch.uint8, device=dev)
            f16 = (torch.randint(0, 1021, (FRAMES,) + size + (3,), dtype=torch.int16, device=dev).to(torch.float16) / 4)
            frames, out = (u8, torch.empty_like(f16)) if kind == "widen" else (f16, torch.empty_like(u8))
            a = torch.empty((FRAMES, mb // 2), dtype=torch.uint8, device=dev)
            b = torch.empty_like(a)
            plans = [pc.Widen(dev, size, force_general=force) if kind == "widen" else pc.Narrow(dev, size, dither=dither, force_general=force)
                     for force in (False, True)]
            best = {}
            for _ in range(ROUNDS):
                for key, fn in (("vec", lambda: plans[0].run(frames, out=out)), ("general", lambda: plans[1].run(frames, out=out)),
                                ("copy", lambda: b.copy_(a))):
                    us = _timed(fn)
                    best[key] = min(us, best.get(key, us))
            assert plans[0].plan()["depth"].endswith("vec>") and plans[1].plan()["depth"].endswith("general>")
            for key, label in (("vec", plans[0].plan()["depth"]), ("general", plans[1].plan()["depth"]), ("copy", "device-to-device copy of equal traffic")):
                print(f"{name:6s} {label:40s} {best[key]:8.1f} us/frame {mb / best[key] / 1e3:6.0f} GB/s of {mb / 1e6:5.1f} MB"
                      + ("" if key == "copy" else f"   {best[key] / best['copy']:5.2f} x the copy"), flush=True)
            for p in plans:
                p.close()
            del u8, f16, frames, out, a, b
            torch.cuda.synchronize()


def report(directory):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        print(f"no *kernel_trace.csv under {directory}", file=sys.stderr)
        return 2
    rows = []
    for f in files:
        for row in csv.DictReader(open(f)):
            if "k_widen" in row["Kernel_Name"] or "k_narrow" in row["Kernel_Name"]:
                rows.append((int(row["Start_Timestamp"]), "general" if "general" in row["Kernel_Name"] else "vec",
                             int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    rows.sort()
    pos = 0
    for name, size in SIZES:
        for kind, dither in KINDS:
            times = {"vec": [], "general": []}
            for _ in range(ROUNDS):
                for path in ("vec", "general"):
                    for batch in range(WARM + RUNS):
                        if pos >= len(rows) or rows[pos][1] != path:
                            print(f"trace does not follow the run's order at dispatch {pos}: expected {path}", file=sys.stderr)
                            return 2
                        if batch >= WARM:
                            times[path].append(rows[pos][2])
                        pos += 1
            mb = moved_bytes(size)
            for path, v in times.items():
                us = sum(v) / len(v) / 1e3 / FRAMES
                print(f"{name:6s} {kind:6s} {dither:7s} {path:8s} {us:8.1f} us/frame {mb / us / 1e3:6.0f} GB/s of {mb / 1e6:5.1f} MB   "
                      f"({len(v)} dispatches of {FRAMES} frames, min {min(v) / 1e3 / FRAMES:.1f}, max {max(v) / 1e3 / FRAMES:.1f})")
    if pos != len(rows):
        print(f"{len(rows) - pos} depth dispatches beyond the run's sequence", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "report":
        sys.exit(report(sys.argv[2]))
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run()
        sys.exit(0)
    print(__doc__)
    sys.exit(2)
