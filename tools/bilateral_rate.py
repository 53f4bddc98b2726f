#!/usr/bin/env python3
"""Rate of the bilateral kernels (mi_blur_enqueue_bilateral) on one GPU, beside the median of the same radius
(mi_blur_enqueue_median, radius 1..7): the existing filter with the same window and non-linear per-window work, measured in
the same run.

    python tools/bilateral_rate.py [--seconds 0.5] [--repeats 5] [--json FILE]

Per point: launches back to back on one stream for at least --seconds between two events (after a warm-up that also
sizes the run), --repeats times; reported as the MEDIAN ms per launch (and the smallest and largest), output bytes per
second, taps per second (output bytes x (2r+1)^2) and the ratio of the bilateral's time to the median's.  Device-resident
buffers of random bytes.  Shapes: one 8192x8192x3 image and one 1920x1080x3 frame.  Radii 1, 2, 3, 5, 8, Gaussian tables
(sigma_space r/2, sigma_range 25).
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
RADII = (1, 2, 3, 5, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    import torch
    pkg = entry.load_package()
    L = pkg.lib()
    torch.cuda.set_device(0)
    rows = []
    print(f"{torch.cuda.get_device_name(0)}; >= {args.seconds:.1f} s of back-to-back launches per point, {args.repeats} times, median")
    print(f"{'shape':12s} {'kernel':18s} {'r':>2s} {'launches':>8s} {'ms med':>9s} {'ms min':>9s} {'ms max':>9s} {'GB/s out':>9s} {'Gtap/s':>8s} {'vs median':>9s}  kernel name")
    for name, n, h, w, c in SHAPES:
        d_in = torch.randint(0, 256, (n, h, w, c), dtype=torch.uint8, device="cuda")
        d_out = torch.empty_like(d_in)
        s = torch.cuda.current_stream()
        out_bytes = d_in.numel()
        for r in RADII:
            k = pkg.Bilateral.gauss(0.0, 25.0, r)
            timed = {}
            for kname in ("bilateral", "median"):
                if kname == "median" and r > pkg.MEDIAN_MAX_RADIUS:
                    continue

                def go():
                    if kname == "bilateral":
                        rc = L.mi_blur_enqueue_bilateral(d_in.data_ptr(), d_out.data_ptr(), w, h, c, n, C.byref(k), s.cuda_stream)
                    else:
                        rc = L.mi_blur_enqueue_median(d_in.data_ptr(), d_out.data_ptr(), w, h, c, r, n, s.cuda_stream)
                    pkg.check(rc, kname)
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
                timed[kname] = med
                gbs = out_bytes / (med * 1e-3) / 1e9
                taps = out_bytes * (2 * r + 1) ** 2 / (med * 1e-3) / 1e9
                ratio = f"{timed['bilateral'] / med:9.3f}" if kname == "median" else f"{'':9s}"
                print(f"{name:12s} {kname:18s} {r:2d} {reps:8d} {med:9.3f} {min(ms):9.3f} {max(ms):9.3f} {gbs:9.1f} {taps:8.1f} {ratio}  {kern}", flush=True)
                rows.append({"shape": name, "kernel": kname, "r": r, "launches": reps, "ms_median": round(med, 4), "ms_all": [round(m, 4) for m in ms],
                             "out_gb_s": round(gbs, 2), "gtap_s": round(taps, 2), "kernel_name": kern,
                             "bilateral_over_median": round(timed["bilateral"] / med, 4) if kname == "median" else None})
        del d_in, d_out
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
