#!/usr/bin/env python3
"""Rate of the median kernels (mi_blur_enqueue_median) on one GPU, beside the fixed radius-1 kernel (mi_blur_enqueue),
and of the CPU device's median (mi_blur_cpu_run_median) on 16 threads.

    python tools/median_rate.py [--seconds 1.0] [--json FILE]

Per GPU point: launches back to back on one stream for at least --seconds between two events (after a warm-up that also
sizes the run), reported as us per launch and algorithmic TB/s (input + output bytes once each).  Shapes: one
8192x8192x3 image, and a batch of 8 1920x1080x3 frames.  Radii 1, 2, 3 and 7, and mi_blur_enqueue radius 1 for scale.
CPU point: the 8 x 1080p batch at radius 1, 2, 3 and 7, wall time of one call (best of 3).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

SHAPES = [("8192x8192x3", 1, 8192, 8192, 3), ("1920x1080x3 x8", 8, 1080, 1920, 3)]
RADII = [1, 2, 3, 7]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    import torch
    pkg = entry.load_package()
    L = pkg.lib()
    torch.cuda.set_device(0)
    rows = []
    print(f"{torch.cuda.get_device_name(0)}; >= {args.seconds:.1f} s of back-to-back launches per point")
    print(f"{'shape':16s} {'kernel':28s} {'launches':>8s} {'us/launch':>10s} {'TB/s':>6s}  kernel name")
    for name, n, h, w, c in SHAPES:
        d_in = torch.randint(0, 256, (n, h, w, c), dtype=torch.uint8, device="cuda")
        d_out = torch.empty_like(d_in)
        s = torch.cuda.current_stream()
        nbytes = 2 * d_in.numel()
        for r in RADII + [0]:
            kname = f"median {2 * r + 1}x{2 * r + 1} (radius {r})" if r else "mi_blur_enqueue radius 1"

            def go():
                if r == 0:
                    rc = L.mi_blur_enqueue(d_in.data_ptr(), d_out.data_ptr(), w, h, c, 1, n, s.cuda_stream)
                else:
                    rc = L.mi_blur_enqueue_median(d_in.data_ptr(), d_out.data_ptr(), w, h, c, r, n, s.cuda_stream)
                pkg.check(rc, kname)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            go()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(3):
                go()
            e1.record()
            torch.cuda.synchronize()
            per = e0.elapsed_time(e1) / 3
            reps = max(5, int(args.seconds * 1e3 / max(per, 1e-3)) + 1)
            e0.record()
            for _ in range(reps):
                go()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            us = ms * 1e3 / reps
            kern = L.mi_blur_last_kernel().decode()
            tbs = nbytes / (us * 1e-6) / 1e12
            print(f"{name:16s} {kname:28s} {reps:8d} {us:10.1f} {tbs:6.3f}  {kern}", flush=True)
            rows.append({"device": "gpu", "shape": name, "kernel": kname, "radius": r, "launches": reps,
                         "total_ms": round(ms, 1), "us_per_launch": round(us, 2), "tb_s": round(tbs, 4), "kernel_name": kern})
        del d_in, d_out
        torch.cuda.empty_cache()
    # the CPU device on the 1080p batch
    n, h, w, c = 8, 1080, 1920, 3
    host = np.random.default_rng(0).integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    out = np.empty_like(host)
    print(f"\nmi_blur_cpu_run_median, 16 threads, {n} x {w}x{h}x{c} (best of 3 calls)")
    for r in RADII:
        best = 1e30
        for _ in range(3):
            t0 = time.perf_counter()
            pkg.check(L.mi_blur_cpu_run_median(host.ctypes.data, out.ctypes.data, w, h, c, r, n, 16), "cpu median")
            best = min(best, time.perf_counter() - t0)
        gbs = 2 * host.size / best / 1e9
        print(f"radius {r}: {best * 1e3:9.1f} ms per batch  {gbs:7.3f} GB/s  {n / best:8.1f} frames/s", flush=True)
        rows.append({"device": "cpu16", "shape": "1920x1080x3 x8", "radius": r, "ms_per_batch": round(best * 1e3, 2),
                     "gb_s": round(gbs, 4)})
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
