"""Dev tool (GPU box): what the filtered resampler (include/crtfx_resample.h) costs per frame — bicubic and Lanczos, uint8 and half frames,
fused path and general path, the half frames with the two-int32 accumulator and with the int64 one — for the three resizes a user of
process_frames(deliver_size=, in_size=) meets — 4K -> 1080p, 1080p -> 4K, 8K -> 4K — next to two yardsticks measured in the same run: the
BILINEAR stages' fused kernels for the same pair (k_ingest_fused on uint8 frames, k_resize16_fused on half ones) and a device-to-device
copy of equal traffic.

    python tools/resample_kernel_times.py run                    # HIP-event times per frame (launch gaps included) + the copies
    rocprofv3 --kernel-trace --stats -d DIR -o resample --output-format csv -- python tools/resample_kernel_times.py run
    python tools/resample_kernel_times.py report DIR             # kernel time per frame from the trace, next to the bytes each resize moves

`run` launches, per resize, the configurations of `configs()` in order, WARM + RUNS batches of FRAMES frames each; `report` walks the
trace's dispatches in that order, drops each WARM part, and prints mean kernel time per frame, (source + destination bytes) / time, and
the ratio to the BILINEAR kernel of the same pair and sample type.  The copy is torch's `copy_` of a buffer of half the resize's traffic
(it is read and written), timed with HIP events over RUNS back-to-back copies."""
import csv
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAIRS = [("4K -> 1080p", (2160, 3840), (1080, 1920)), ("1080p -> 4K", (1080, 1920), (2160, 3840)), ("8K -> 4K", (4320, 7680), (2160, 3840))]
FRAMES, WARM, RUNS = 4, 3, 20
FUSED, GENERAL = ["k_resample_fused"], ["k_resample_h", "k_resample_v"] * FRAMES      # behind a fused plan the general path's scratch holds one frame


def configs():
    """(label, sample type, filter or None for the BILINEAR stage, force_general, acc64, the kernels one batch dispatches) in run order."""
    out = []
    for px in ("uint8", "half"):
        out.append((f"{px} bilinear fused", px, None, 0, 0, ["k_ingest_fused" if px == "uint8" else "k_resize16_fused"]))
        for filt in ("bicubic", "lanczos"):
            out.append((f"{px} {filt} fused", px, filt, 0, 0, FUSED))
            out.append((f"{px} {filt} general", px, filt, 1, 0, GENERAL))
            if px == "half":
                out.append((f"{px} {filt} fused i64", px, filt, 0, 1, FUSED))
                out.append((f"{px} {filt} general i64", px, filt, 1, 1, GENERAL))
    return out


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
        frames = {"uint8": torch.randint(0, 256, (FRAMES,) + src + (3,), dtype=torch.uint8, device=dev)}
        frames["half"] = (frames["uint8"].to(torch.float32) + torch.rand((FRAMES,) + src + (3,), device=dev) - 0.5).to(torch.float16)
        outs = {"uint8": torch.empty((FRAMES,) + dst + (3,), dtype=torch.uint8, device=dev),
                "half": torch.empty((FRAMES,) + dst + (3,), dtype=torch.float16, device=dev)}
        for label, px, filt, force, acc64, _ in configs():
            if filt is None:
                plan = pc.IngestResize(dev, src, dst) if px == "uint8" else pc.ResizeHalf(dev, src, dst)
                key = "ingest" if px == "uint8" else "resize16"
            else:
                plan = pc.Resample(dev, src, dst, filter=filt, dtype=frames[px].dtype)
                plan.set_option(_lib.RESAMPLE_OPT_FORCE_GENERAL, force)
                if acc64:
                    plan.set_option(_lib.RESAMPLE_OPT_ACC64, 1)
                key = "resample"
                if not force and not plan.plan()[key].startswith("k_resample_fused"):
                    raise SystemExit(f"{name} {label}: no tile fits, the trace would not follow configs()")
            us = _timed(lambda: plan.run(frames[px], out=outs[px]))
            mb = moved_bytes(src, dst, 1 if px == "uint8" else 2)
            print(f"{name:12s} {label:26s} {plan.plan()[key]:44s} {us:9.1f} us/frame (HIP events, launch gaps included)  "
                  f"{mb / us / 1e3:7.0f} GB/s of {mb / 1e6:.1f} MB source + destination", flush=True)
            plan.close()
        del frames, outs
        for what, itemsize in (("uint8", 1), ("half", 2)):
            mb = moved_bytes(src, dst, itemsize)
            a = torch.empty((FRAMES, mb // 2), dtype=torch.uint8, device=dev)
            b = torch.empty_like(a)
            us = _timed(lambda: b.copy_(a))
            print(f"{name:12s} {what + ' copy':26s} {'device-to-device copy of equal traffic':44s} {us:9.1f} us/frame (HIP events, launch gaps included)  "
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
            m = re.search(r"\b(k_(?:resample|resize16|ingest)_(?:fused|h|v))\b", row["Kernel_Name"])
            if m:
                rows.append((int(row["Start_Timestamp"]), m.group(1), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    rows.sort()
    pos = 0
    for name, src, dst in PAIRS:
        base = {}
        for label, px, filt, force, acc64, seq in configs():
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
            if filt is None:
                base[px] = total
            mb = moved_bytes(src, dst, 1 if px == "uint8" else 2)
            detail = " + ".join(f"{k} {per_frame[k]:.1f} us ({len(v)} dispatches, min {min(v) / 1e3 / div:.1f}, max {max(v) / 1e3 / div:.1f})" for k, v in times.items())
            print(f"{name:12s} {label:26s} {total:8.1f} us/frame  {mb / total / 1e3:7.0f} GB/s of {mb / 1e6:.1f} MB  {total / base[px]:5.2f} x bilinear   [{detail}]")
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
