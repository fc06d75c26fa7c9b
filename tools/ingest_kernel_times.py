"""Dev tool (GPU box): what the ingest kernels (include/crtfx_ingest.h) cost per frame, fused path and general path, for the three resizes a
user of process_frames meets: 1080p -> 4K, 720p -> 1080p, 4K -> 1080p.

    python tools/ingest_kernel_times.py run                      # HIP-event times per frame + this box's copy ceiling (bench.copy_ceiling)
    rocprofv3 --kernel-trace --stats -d DIR -o ingest --output-format csv -- python tools/ingest_kernel_times.py run --no-ceiling
    python tools/ingest_kernel_times.py report DIR               # kernel time per frame from the trace, next to the bytes each resize moves

`run` launches, per resize and path, WARM + RUNS batches of FRAMES frames; `report` walks the trace's dispatches in that order, drops each
WARM part, and prints mean kernel time per frame and (source + destination bytes) / time."""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAIRS = [("1080p -> 4K", (1080, 1920), (2160, 3840)), ("720p -> 1080p", (720, 1280), (1080, 1920)), ("4K -> 1080p", (2160, 3840), (1080, 1920))]
FRAMES, WARM, RUNS = 4, 3, 20


def moved_bytes(src, dst):
    return 3 * (src[0] * src[1] + dst[0] * dst[1])


def run(ceiling=True):
    import torch
    import pythoncrt_amd as pc
    from pythoncrt_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    if ceiling:
        import bench
        print(f"copy ceiling of this box (bench.copy_ceiling, 1 GiB device-to-device, read + write): {bench.copy_ceiling(dev)} GB/s", flush=True)
    for name, src, dst in PAIRS:
        frames = torch.randint(0, 256, (FRAMES,) + src + (3,), dtype=torch.uint8, device=dev)
        out = torch.empty((FRAMES,) + dst + (3,), dtype=torch.uint8, device=dev)
        for force in (0, 1):
            plan = pc.IngestResize(dev, src, dst)
            plan.set_option(_lib.INGEST_OPT_FORCE_GENERAL, force)
            for _ in range(WARM):
                plan.run(frames, out=out)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(RUNS):
                plan.run(frames, out=out)
            e1.record()
            e1.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / (RUNS * FRAMES)
            print(f"{name:14s} {plan.plan()['ingest']:36s} {us:9.1f} us/frame (HIP events, launch gaps included)  "
                  f"{moved_bytes(src, dst) / us / 1e3:7.0f} GB/s of {moved_bytes(src, dst) / 1e6:.1f} MB source + destination", flush=True)
            plan.close()


def report(directory):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        print(f"no *kernel_trace.csv under {directory}", file=sys.stderr)
        return 2
    rows = []
    for f in files:
        for row in csv.DictReader(open(f)):
            if "k_ingest" in row["Kernel_Name"]:
                rows.append((int(row["Start_Timestamp"]), "k_ingest_" + row["Kernel_Name"].split("k_ingest_")[1].split("(")[0],
                             int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    rows.sort()
    # the dispatches in the order `run` issues them (grids repeat between the resizes, the order does not): per resize WARM + RUNS fused grids of
    # FRAMES frames, then WARM + RUNS batches of FRAMES x (k_ingest_h, k_ingest_v) — behind a fused plan the general path's scratch holds one frame
    pos = 0
    for name, src, dst in PAIRS:
        for path, seq in (("fused", ["k_ingest_fused"]), ("general", ["k_ingest_h", "k_ingest_v"] * FRAMES)):
            times = {k: [] for k in seq}
            for batch in range(WARM + RUNS):
                for k in seq:
                    if pos >= len(rows) or rows[pos][1] != k:
                        print(f"trace does not follow the run's order at dispatch {pos}: expected {k}", file=sys.stderr)
                        return 2
                    if batch >= WARM:
                        times[k].append(rows[pos][2])
                    pos += 1
            per_frame = {k: sum(v) / len(v) / 1e3 / (FRAMES if path == "fused" else 1) for k, v in times.items()}
            total = sum(per_frame.values())
            detail = " + ".join(f"{k} {per_frame[k]:.1f} us ({len(v)} dispatches, min {min(v) / 1e3 / (FRAMES if path == 'fused' else 1):.1f}, "
                                f"max {max(v) / 1e3 / (FRAMES if path == 'fused' else 1):.1f})" for k, v in times.items())
            print(f"{name:14s} {path:8s} {total:8.1f} us/frame  {moved_bytes(src, dst) / total / 1e3:7.0f} GB/s of {moved_bytes(src, dst) / 1e6:.1f} MB   [{detail}]")
    if pos != len(rows):
        print(f"{len(rows) - pos} ingest dispatches beyond the run's sequence", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "report":
        sys.exit(report(sys.argv[2]))
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run(ceiling="--no-ceiling" not in sys.argv)
        sys.exit(0)
    print(__doc__)
    sys.exit(2)
