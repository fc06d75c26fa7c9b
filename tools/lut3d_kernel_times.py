"""Dev tool (GPU box): what the 3D LUT stage (include/crtfx_lut3d.h) costs per frame — cube sizes 17, 33 and 65; uint8 and half frames;
1080p and 4K; the cube in LDS (`lds`) and in device memory (`global`); four pixels per lane (`vec`) and one (`general`) — next to a
yardstick measured in the same run: a device-to-device copy of the same traffic (a frame is read and a frame is written).  Which table
path is the default for an N is decided by these figures (the header's timing block quotes them): `lds` only where it is the faster
one at both sizes.

    python tools/lut3d_kernel_times.py run [OUT]                # HIP-event times per frame (launch gaps included) + the copies + ratios

`run` launches, per size, sample type and N, ROUNDS rounds of (each path, copy), each WARM + RUNS batches of FRAMES frames timed with HIP
events over the RUNS back-to-back batches, and prints the best round of each (the rounds alternate so that a neighbour's load on the
machine hits all of them) and the ratios to the copy.  The copy is torch's `copy_` of a buffer of a frame's bytes (it is read and
written).  The whole output also goes to OUT (default profiles/lut3d.txt)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [("1080p", (1080, 1920)), ("4K", (2160, 3840))]
CUBES = [17, 33, 65]
DTYPES = ["uint8", "float16"]
FRAMES, WARM, RUNS, ROUNDS = 8, 3, 20, 3


def moved_bytes(size, dtype):
    return size[0] * size[1] * 3 * (1 if dtype == "uint8" else 2) * 2


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


def run(out_path):
    import numpy as np
    import torch
    import pythoncrt_amd as pc
    dev = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    log = open(out_path, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()
    say(f"batches of {FRAMES} frames, {WARM} warm-up + {RUNS} timed batches per figure, best of {ROUNDS} alternating rounds; us per frame from HIP "
        "events (launch gaps included); traffic = a frame read + a frame written; random cubes, random frames")
    verdict = {}
    for name, size in SIZES:
        for dtype in DTYPES:
            tdt = getattr(torch, dtype)
            mb = moved_bytes(size, dtype)
            if dtype == "uint8":
                frames = torch.randint(0, 256, (FRAMES,) + size + (3,), dtype=torch.uint8, device=dev)
            else:
                frames = torch.randint(0, 1021, (FRAMES,) + size + (3,), dtype=torch.int16, device=dev).to(torch.float16) / 4
            out = torch.empty_like(frames)
            a = torch.empty((FRAMES, mb // 2), dtype=torch.uint8, device=dev)
            b = torch.empty_like(a)
            for n in CUBES:
                rng = np.random.default_rng(n)
                cube = pc.Cube(n, rng.random((n, n, n, 3)))
                plans = {}
                for table in ("lds", "global"):
                    for walk in ("vec", "general"):
                        p = pc.Lut3D(dev, size, cube, dtype=tdt, force_general=walk == "general")
                        p.force_global = table == "global"
                        if p.plan()["lut3d"].split(",")[1] != table:           # N = 65: there is no lds path
                            p.close()
                            continue
                        plans[(table, walk)] = p
                best = {}
                for _ in range(ROUNDS):
                    for key, fn in [(k, (lambda p=p: p.run(frames, out=out))) for k, p in plans.items()] + [("copy", lambda: b.copy_(a))]:
                        us = _timed(fn)
                        best[key] = min(us, best.get(key, us))
                for key, p in plans.items():
                    assert p.plan()["lut3d"].split("<")[1].rstrip(">").split(",")[1:] == list(key), p.last_plan()
                    say(f"{name:6s} {dtype:8s} N={n:2d} {p.plan()['lut3d']:30s} {best[key]:8.1f} us/frame {mb / best[key] / 1e3:6.0f} GB/s of {mb / 1e6:5.1f} MB"
                        f"   {best[key] / best['copy']:5.2f} x the copy")
                    p.close()
                say(f"{name:6s} {dtype:8s} N={n:2d} {'device-to-device copy of equal traffic':30s} {best['copy']:8.1f} us/frame {mb / best['copy'] / 1e3:6.0f} GB/s")
                if ("lds", "vec") in best:
                    verdict.setdefault(n, []).append((name, dtype, best[("lds", "vec")], best[("global", "vec")]))
            del frames, out, a, b
            torch.cuda.synchronize()
    for n, rows in sorted(verdict.items()):
        wins = all(l < g for _, _, l, g in rows)
        say(f"N={n}: lds is {'the faster table path in every case: the default' if wins else 'NOT the faster path in every case: global is the default'} ("
            + ", ".join(f"{name} {dtype} {l:.1f} vs {g:.1f}" for name, dtype, l, g in rows) + ")")
    log.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "lut3d.txt"))
        sys.exit(0)
    print(__doc__)
    sys.exit(2)
