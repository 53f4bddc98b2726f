#!/usr/bin/env python3
"""Rate of the convolution kernels (mi_blur_enqueue_conv) on one GPU, beside two kernels this tool does not touch,
measured in the same run: the bilateral filter (mi_blur_enqueue_bilateral, radii 1, 2, 3, 5) and the 3x3 blur
(mi_blur_enqueue, radius 1).

    python tools/conv_rate.py [--seconds 0.3] [--repeats 5] [--json FILE]

Per point: launches back to back on one stream for at least --seconds between two events (after a warm-up that also
sizes the run), --repeats times; reported as the MEDIAN ms per launch (and the smallest and largest), output bytes per
second and taps per second (output bytes x window taps; MAG counts both tables).  Device-resident buffers of random bytes.
Shapes: one 8192x8192x3 image and one 1920x1080x3 frame.  Convolution: square random kernels (taps -4..4, no zeros) of
radius 1, 2, 3, 5, 7 in SAT mode, and the Sobel magnitude (MAG, radius 1).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

SHAPES = [("8192x8192x3", 1, 8192, 8192, 3), ("1920x1080x3", 1, 1080, 1920, 3)]
CONV_RADII = (1, 2, 3, 5, 7)
BILATERAL_RADII = (1, 2, 3, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    pkg = entry.load_package()
    L = pkg.lib()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(7)
    rows = []
    print(f"{torch.cuda.get_device_name(0)}; >= {args.seconds:.1f} s of back-to-back launches per point, {args.repeats} times, median")
    print(f"{'shape':12s} {'kernel':14s} {'r':>2s} {'launches':>8s} {'ms med':>9s} {'ms min':>9s} {'ms max':>9s} {'GB/s out':>9s} {'Gtap/s':>8s}  kernel name")
    for name, n, h, w, c in SHAPES:
        d_in = torch.randint(0, 256, (n, h, w, c), dtype=torch.uint8, device="cuda")
        d_out = torch.empty_like(d_in)
        s = torch.cuda.current_stream().cuda_stream
        pin, pout = d_in.data_ptr(), d_out.data_ptr()
        out_bytes = d_in.numel()
        points = []
        for r in CONV_RADII:
            taps = rng.integers(1, 5, size=(2 * r + 1, 2 * r + 1)) * rng.choice((-1, 1), size=(2 * r + 1, 2 * r + 1))
            k = pkg.Conv.from_taps(taps.tolist(), shift=4, bias=8)
            points.append(("conv sat", r, (2 * r + 1) ** 2, lambda k=k: L.mi_blur_enqueue_conv(pin, pout, w, h, c, n, C.byref(k), s)))
        k = pkg.Conv.preset("sobel_mag")
        points.append(("conv mag", 1, 18, lambda k=k: L.mi_blur_enqueue_conv(pin, pout, w, h, c, n, C.byref(k), s)))
        for r in BILATERAL_RADII:
            b = pkg.Bilateral.gauss(0.0, 25.0, r)
            points.append(("bilateral", r, (2 * r + 1) ** 2, lambda b=b: L.mi_blur_enqueue_bilateral(pin, pout, w, h, c, n, C.byref(b), s)))
        points.append(("blur 3x3", 1, 9, lambda: L.mi_blur_enqueue(pin, pout, w, h, c, 1, n, s)))
        for kname, r, ntaps, call in points:
            def go():
                pkg.check(call(), kname)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(2):
                go()
            e0.record()
            for _ in range(4):
                go()
            e1.record()
            torch.cuda.synchronize()
            per = e0.elapsed_time(e1) / 4
            reps = max(5, int(args.seconds * 1e3 / max(per, 1e-3)) + 1)
            ms = []
            for _ in range(args.repeats):
                e0.record()
                for _ in range(reps):
                    go()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / reps)
            kern = L.mi_blur_last_kernel().decode()
            med = statistics.median(ms)
            gbs = out_bytes / (med * 1e-3) / 1e9
            gtaps = out_bytes * ntaps / (med * 1e-3) / 1e9
            print(f"{name:12s} {kname:14s} {r:2d} {reps:8d} {med:9.3f} {min(ms):9.3f} {max(ms):9.3f} {gbs:9.1f} {gtaps:8.1f}  {kern}", flush=True)
            rows.append({"shape": name, "kernel": kname, "r": r, "launches": reps, "ms_median": round(med, 4), "ms_all": [round(m, 4) for m in ms],
                         "out_gb_s": round(gbs, 2), "gtap_s": round(gtaps, 2), "kernel_name": kern})
        del d_in, d_out
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
