"""Dev tool (GPU box): what the egress kernels (include/crtfx_egress.h) cost per frame — both layouts, vec and general path, 1080p and 4K,
batches of 8 — next to the yardstick of this box: a device-to-device copy of 2.25 * h * w bytes per frame in the same batches (a copy moves
every byte twice: the same 4.5 bytes per pixel of traffic as 3 in + 1.5 out).  And the end of the pipeline with and without the stage.

    python tools/egress_kernel_times.py run                      # HIP-event times per frame, the copy yardstick, the shader clock while it ran
    python tools/egress_kernel_times.py e2e [--repeats R]        # process_frames and the CLI at 4K: rgb24 against yuv420p / nv12
    rocprofv3 --kernel-trace --stats -d DIR -o egress --output-format csv -- python tools/egress_kernel_times.py run --no-clock

`run` launches, per size / layout / path, WARM + RUNS batches of FRAMES frames on one stream between two events."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [("1080p", 1080, 1920), ("4K", 2160, 3840)]
FRAMES, WARM, RUNS = 8, 5, 60


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
    return e0.elapsed_time(e1) * 1e3 / (RUNS * FRAMES)          # us per frame, launch gaps included


def run(clock=True):
    import torch
    import pythoncrt_amd as pc
    from pythoncrt_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    tel = None
    if clock:
        import bench
        tel = bench.GpuTelemetry(dev)
        tel.start()
    print(f"device: {torch.cuda.get_device_name(dev)}; batches of {FRAMES} frames, {WARM} warm-up + {RUNS} timed batches per row, HIP events on one stream", flush=True)
    for name, h, w in SIZES:
        nbytes = int(2.25 * h * w)
        a = torch.randint(0, 256, (FRAMES, nbytes), dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        copy_us = _timed(lambda: b.copy_(a))
        print(f"{name:6s} device-to-device copy of 2.25*h*w = {nbytes / 1e6:.2f} MB per frame: {copy_us:8.1f} us/frame = {2 * nbytes / copy_us / 1e3:6.0f} GB/s read + write",
              flush=True)
        del a, b
        frames = torch.randint(0, 256, (FRAMES, h, w, 3), dtype=torch.uint8, device=dev)
        for layout in ("yuv420p", "nv12"):
            for force in (0, 1):
                plan = pc.EgressYuv(dev, (h, w), layout=layout)
                plan.set_option(_lib.EGRESS_OPT_FORCE_GENERAL, force)
                out = torch.empty((FRAMES, plan.frame_bytes), dtype=torch.uint8, device=dev)
                us = _timed(lambda: plan.run(frames, out=out))
                moved = 3 * h * w + plan.frame_bytes
                print(f"{name:6s} {plan.plan()['egress']:34s} {us:8.1f} us/frame = {moved / us / 1e3:6.0f} GB/s of {moved / 1e6:.1f} MB in + out; "
                      f"{us / copy_us:5.2f} x the copy", flush=True)
                plan.close()
        del frames
    if tel is not None:
        print(f"shader clock / power while it ran: {tel.stop()}", flush=True)


def e2e(repeats=3):
    """process_frames (in-memory iterator, a writer that does nothing) and the CLI (file to file on the temporary directory, --io staged) at
    4K with the reference CLI's default settings: frames/s per output format, `repeats` runs each."""
    import subprocess
    import tempfile
    import numpy as np
    import pythoncrt_amd as pc
    h, w, n = 2160, 3840, 64
    rng = np.random.default_rng(0)
    base = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(8)]
    fmts = [f for f in ("rgb24", "yuv420p", "nv12") if f == "rgb24" or hasattr(pc, "EgressYuv")]
    for fmt in fmts:
        kw = {} if fmt == "rgb24" else {"out_pix_fmt": fmt}
        pc.process_frames(iter(base), lambda a: None, w, h, 30, 8, noise_seed=1, **kw)
        rates = []
        for _ in range(repeats):
            t = time.perf_counter()
            k = pc.process_frames((base[i % 8] for i in range(n)), lambda a: None, w, h, 30, n, noise_seed=1, **kw)
            rates.append(k / (time.perf_counter() - t))
        print(f"process_frames 4K {fmt:8s}: " + ", ".join(f"{r:.0f}" for r in rates) + f" frames/s ({n} frames per run, set-up of the call included)", flush=True)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory(dir=os.environ.get("CRTFX_TMP") or None) as tmp:
        src = os.path.join(tmp, "in.rgb")
        with open(src, "wb") as f:
            for i in range(n):
                f.write(base[i % 8].tobytes())
        for fmt in fmts:
            rates = []
            for _ in range(repeats + 1):                         # the first run warms the page cache and is dropped
                cmd = [sys.executable, "-m", "pythoncrt_amd.cli", "--input", src, "--output", os.path.join(tmp, "out.raw"), "--width", str(w), "--height", str(h),
                       "--fps", "30", "--noise-seed", "1", "--staging-report"] + ([] if fmt == "rgb24" else ["--out-pix-fmt", fmt])
                r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    print(r.stderr[-2000:], file=sys.stderr)
                    return 2
                line = [ln for ln in r.stderr.splitlines() if "staging: pipeline" in ln][-1]
                rates.append(float(line.split(" = ")[1].split()[0]))
                size = os.path.getsize(os.path.join(tmp, "out.raw"))
            print(f"CLI 4K file -> file {fmt:8s}: " + ", ".join(f"{r:.0f}" for r in rates[1:]) + f" frames/s (first read issued ... last batch written; {n} frames, "
                  f"output {size / n / 1e6:.1f} MB per frame)", flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run(clock="--no-clock" not in sys.argv)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "e2e":
        sys.exit(e2e(int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 3))
    print(__doc__)
    sys.exit(2)
