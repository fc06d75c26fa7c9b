"""Dev tool (GPU box): what the field-paired 4:2:0 source kernels (include/crtfx_field420.h) cost per frame — every layout, vec and general
path, chroma replicate and left, 480 x 720, 1080p and 4K — next to two yardsticks taken in the same run: the untouched
k_unpack_sited<layout,vec> at siting left, which moves the same bytes with the same tap count, and a device-to-device copy of the same
traffic per frame in the same batches.  A frame of frame_bytes and its RGB frame are frame_bytes + rgb_bytes of traffic (4.5 * h * w for
the 8-bit layouts, 9 for the 10-bit ones); a copy moves every byte twice, so the yardstick copies half of that per frame.

    python tools/field420_kernel_times.py run [--no-clock] [--out FILE]     # prints, and writes profiles/field420.txt (or FILE)

Per size and row it launches WARM + a per-size number of batches of FRAMES frames on one stream between two HIP events, so that every timed
window lasts about 0.1 s or more; the rows of one size are taken ROUNDS times in turn (the copies, then every kernel build) so that a drift
of the clock shows as spread between the rounds, and the median per row is printed beside the smallest and largest.  It measures throughput
against the sited vec build and the copy of equal traffic, nothing else."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [("480i", 480, 720, 8000), ("1080i", 1080, 1920, 3000), ("4K", 2160, 3840, 800)]      # name, h, w, timed batches per row and round
FRAMES, WARM, ROUNDS = 8, 3, 3


def _timed(fn, runs):
    import torch
    for _ in range(WARM):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(runs):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (runs * FRAMES)          # us per frame, launch gaps included


def run(clock=True, out_path=None):
    import torch
    import pythoncrt_amd as pc
    from pythoncrt_amd import field420, formats
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device visible: nothing is measured without one")
    dev = torch.device("cuda", torch.cuda.current_device())
    out_path = out_path or os.path.join(ROOT, "profiles", "field420.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    log = open(out_path, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()
    tel = None
    if clock:
        import bench
        tel = bench.GpuTelemetry(dev)
        tel.start()
    say(f"device: {torch.cuda.get_device_name(dev)}; batches of {FRAMES} frames, {WARM} warm-up + "
        f"{' / '.join(str(s[3]) for s in SIZES)} ({' / '.join(s[0] for s in SIZES)}) timed batches per row and round, {ROUNDS} rounds, HIP events on one stream; "
        "median (min .. max) of the rounds")
    for name, h, w, runs in SIZES:
        rows, keep, copies = [], [], {}                         # (label, traffic, callable, layout, what); traffic in bytes per frame -> (a, b) of its copy
        for layout in field420.LAYOUTS:
            deep = formats.bits(layout) == 10
            fb = field420.frame_bytes(h, w, layout)
            moved = fb + h * w * (6 if deep else 3)
            if moved not in copies:
                a = torch.randint(0, 256, (FRAMES, moved // 2), dtype=torch.uint8, device=dev)
                copies[moved] = (a, torch.empty_like(a))
            packed = torch.randint(0, 256, (FRAMES, fb), dtype=torch.uint8, device=dev)
            out = torch.empty((FRAMES, h, w, 3), dtype=torch.float16 if deep else torch.uint8, device=dev)
            keep.append((packed, out))
            plans = [(pc.UnpackSited(dev, (h, w), layout, siting="left"), False, "sited")]
            plans += [(pc.UnpackField420(dev, (h, w), layout, chroma=chroma), force, chroma) for force in (False, True) for chroma in ("replicate", "left")]
            for plan, force, what in plans:
                plan.force_general = force
                plan.run(packed, out=out)
                key = next(k for k in plan.plan() if k not in ("frames", "siting", "chroma"))
                label = plan.plan()[key] + (" left (the yardstick)" if what == "sited" else f" {what}")
                rows.append((label, moved, (lambda p=plan, s=packed, o=out: p.run(s, out=o)), layout, what))
                keep.append(plan)
        copy_us, times = {m: [] for m in copies}, [[] for _ in rows]
        for _ in range(ROUNDS):
            for m, (a, b) in copies.items():
                copy_us[m].append(_timed(lambda a=a, b=b: b.copy_(a), runs))
            for i, row in enumerate(rows):
                times[i].append(_timed(row[2], runs))
        cmed = {m: statistics.median(v) for m, v in copy_us.items()}
        for m, v in copy_us.items():
            say(f"{name:6s} device-to-device copy of {m / 2 / (h * w):.2f}*h*w = {m / 2e6:.2f} MB per frame: {cmed[m]:8.2f} ({min(v):.2f} .. {max(v):.2f}) us/frame = "
                f"{m / cmed[m] / 1e3:6.0f} GB/s read + write")
        med = [statistics.median(t) for t in times]
        base = {row[3]: med[i] for i, row in enumerate(rows) if row[4] == "sited"}      # the sited vec build of the same layout
        for (label, moved, _, layout, what), t, m in zip(rows, times, med):
            say(f"{name:6s} {label:58s} {m:8.2f} ({min(t):.2f} .. {max(t):.2f}) us/frame = {moved / m / 1e3:6.0f} GB/s of {moved / 1e6:.1f} MB in + out; "
                f"{m / cmed[moved]:5.2f} x the copy" + ("" if what == "sited" else f"; {m / base[layout]:5.2f} x the sited vec build"))
        for item in keep:
            if hasattr(item, "close"):
                item.close()
        del copies, rows, keep
    if tel is not None:
        say(f"shader clock / power while it ran: {tel.stop()}")
    log.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
        run(clock="--no-clock" not in sys.argv, out_path=path)
        sys.exit(0)
    print(__doc__)
    sys.exit(2)
