"""Dev tool (GPU box): what the half resampler (include/crtfx_resize16.h) costs per frame, fused path and general path, for the three
resizes a user of process_frames(deliver_size=) meets — 4K -> 1080p, 1080p -> 4K, 8K -> 4K — next to two yardsticks measured in the same
run: k_ingest_fused on uint8 frames for the same pair, and a device-to-device copy of equal traffic.

    python tools/resize16_kernel_times.py run                    # HIP-event times per frame (launch gaps included) + the copies
    rocprofv3 --kernel-trace --stats -d DIR -o resize16 --output-format csv -- python tools/resize16_kernel_times.py run
    python tools/resize16_kernel_times.py report DIR             # kernel time per frame from the trace, next to the bytes each resize moves

`run` launches, per resize, WARM + RUNS batches of FRAMES frames on the fused path, then on the general path, then on the ingest stage's
fused path (uint8); `report` walks the trace's dispatches in that order, drops each WARM part, and prints mean kernel time per frame and
(source + destination bytes) / time.  The copy is torch's `copy_` of a buffer of half the resize's traffic (it is read and written), timed
with HIP events over RUNS back-to-back copies."""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAIRS = [("4K -> 1080p", (2160, 3840), (1080, 1920)), ("1080p -> 4K", (1080, 1920), (2160, 3840)), ("8K -> 4K", (4320, 7680), (2160, 3840))]
FRAMES, WARM, RUNS = 4, 3, 20


def moved_bytes(src, dst, itemsize):
    return 3 * itemsize * (src[0] * src[1] + dst[0] * dst[1])


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
    from pythoncrt_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    for name, src, dst in PAIRS:
        half = (torch.rand((FRAMES,) + src + (3,), device=dev) * 255.0).to(torch.float16)
        out = torch.empty((FRAMES,) + dst + (3,), dtype=torch.float16, device=dev)
        for force in (0, 1):
            plan = pc.ResizeHalf(dev, src, dst)
            plan.set_option(_lib.RESIZE16_OPT_FORCE_GENERAL, force)
            us = _timed(lambda: plan.run(half, out=out))
            mb = moved_bytes(src, dst, 2)
            print(f"{name:12s} half  {plan.plan()['resize16']:36s} {us:9.1f} us/frame (HIP events, launch gaps included)  "
                  f"{mb / us / 1e3:7.0f} GB/s of {mb / 1e6:.1f} MB source + destination", flush=True)
            plan.close()
        del half, out
        u8 = torch.randint(0, 256, (FRAMES,) + src + (3,), dtype=torch.uint8, device=dev)
        out8 = torch.empty((FRAMES,) + dst + (3,), dtype=torch.uint8, device=dev)
        plan = pc.IngestResize(dev, src, dst)
        us = _timed(lambda: plan.run(u8, out=out8))
        mb = moved_bytes(src, dst, 1)
        print(f"{name:12s} uint8 {plan.plan()['ingest']:36s} {us:9.1f} us/frame (HIP events, launch gaps included)  "
              f"{mb / us / 1e3:7.0f} GB/s of {mb / 1e6:.1f} MB source + destination", flush=True)
        plan.close()
        del u8, out8
        for what, itemsize in (("half", 2), ("uint8", 1)):
            mb = moved_bytes(src, dst, itemsize)
            a = torch.empty((FRAMES, mb // 2), dtype=torch.uint8, device=dev)
            b = torch.empty_like(a)
            us = _timed(lambda: b.copy_(a))
            print(f"{name:12s} {what:5s} {'device-to-device copy of equal traffic':36s} {us:9.1f} us/frame (HIP events, launch gaps included)  "
                  f"{mb / us / 1e3:7.0f} GB/s of {mb / 1e6:.1f} MB read + written", flush=True)
            del a, b
        torch.cuda.synchronize()


def report(directory):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        print(f"no *kernel_trace.csv under {directory}", file=sys.stderr)
        return 2
    rows = []
    for f in files:
        for row in csv.DictReader(open(f)):
            for stem in ("k_resize16_", "k_ingest_"):
                if stem in row["Kernel_Name"]:
                    rows.append((int(row["Start_Timestamp"]), stem + row["Kernel_Name"].split(stem)[1].split("(")[0],
                                 int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    rows.sort()
    # the dispatches in the order `run` issues them: per resize WARM + RUNS fused grids of FRAMES frames, then WARM + RUNS batches of
    # FRAMES x (k_resize16_h, k_resize16_v) — behind a fused plan the general path's scratch holds one frame — then WARM + RUNS grids of k_ingest_fused
    pos = 0
    for name, src, dst in PAIRS:
        for path, seq, itemsize in (("half fused", ["k_resize16_fused"], 2), ("half general", ["k_resize16_h", "k_resize16_v"] * FRAMES, 2),
                                    ("uint8 ingest fused", ["k_ingest_fused"], 1)):
            one_grid = len(seq) == 1
            times = {k: [] for k in seq}
            for batch in range(WARM + RUNS):
                for k in seq:
                    if pos >= len(rows) or rows[pos][1] != k:
                        print(f"trace does not follow the run's order at dispatch {pos}: expected {k}", file=sys.stderr)
                        return 2
                    if batch >= WARM:
                        times[k].append(rows[pos][2])
                    pos += 1
            div = FRAMES if one_grid else 1
            per_frame = {k: sum(v) / len(v) / 1e3 / div for k, v in times.items()}
            total = sum(per_frame.values())
            mb = moved_bytes(src, dst, itemsize)
            detail = " + ".join(f"{k} {per_frame[k]:.1f} us ({len(v)} dispatches, min {min(v) / 1e3 / div:.1f}, max {max(v) / 1e3 / div:.1f})" for k, v in times.items())
            print(f"{name:12s} {path:18s} {total:8.1f} us/frame  {mb / total / 1e3:7.0f} GB/s of {mb / 1e6:.1f} MB   [{detail}]")
    if pos != len(rows):
        print(f"{len(rows) - pos} resize dispatches beyond the run's sequence", file=sys.stderr)
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
