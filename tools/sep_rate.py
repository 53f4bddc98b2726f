#!/usr/bin/env python3
"""Rate of the separable kernels (mi_blur_enqueue_sep) on one GPU, beside the fixed radius-1 kernel (mi_blur_enqueue).

    python tools/sep_rate.py [--seconds 1.0] [--json FILE]

Per point: launches back to back on one stream for at least --seconds between two events (after a warm-up that also
sizes the run), reported as us per launch and algorithmic TB/s (input + output bytes once each).  Shapes: one
8192x8192x3 image, and a batch of 8 1920x1080x3 frames.  Kernels: Gaussian sigma 1, 2, 3, 5 (8-bit taps), the binomial
{1,2,1} through the separable path, and mi_blur_enqueue radius 1 (the fixed 3x3 kernels) for scale.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

SHAPES = [("8192x8192x3", 1, 8192, 8192, 3), ("1920x1080x3 x8", 8, 1080, 1920, 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    import torch
    pkg = entry.load_package()
    L = pkg.lib()
    torch.cuda.set_device(0)
    kernels = [(f"gauss sigma {s}", pkg.gauss_kernel(s)) for s in (1.0, 2.0, 3.0, 5.0)]
    kernels.append(("binomial {1,2,1} (sep path)", pkg.SepKernel.from_taps([1, 2, 1])))
    kernels.append(("mi_blur_enqueue radius 1", None))
    rows = []
    print(f"{torch.cuda.get_device_name(0)}; >= {args.seconds:.1f} s of back-to-back launches per point")
    print(f"{'shape':16s} {'kernel':30s} {'rx':>3s} {'ry':>3s} {'launches':>8s} {'us/launch':>10s} {'TB/s':>6s}  kernel name")
    for name, n, h, w, c in SHAPES:
        d_in = torch.randint(0, 256, (n, h, w, c), dtype=torch.uint8, device="cuda")
        d_out = torch.empty_like(d_in)
        s = torch.cuda.current_stream()
        nbytes = 2 * d_in.numel()
        for kname, k in kernels:
            def go():
                if k is None:
                    rc = L.mi_blur_enqueue(d_in.data_ptr(), d_out.data_ptr(), w, h, c, 1, n, s.cuda_stream)
                else:
                    rc = L.mi_blur_enqueue_sep(d_in.data_ptr(), d_out.data_ptr(), w, h, c, n, C.byref(k), s.cuda_stream)
                pkg.check(rc, kname)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(3):
                go()
            e0.record()
            for _ in range(10):
                go()
            e1.record()
            torch.cuda.synchronize()
            per = e0.elapsed_time(e1) / 10
            reps = max(20, int(args.seconds * 1e3 / max(per, 1e-3)) + 1)
            e0.record()
            for _ in range(reps):
                go()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            us = ms * 1e3 / reps
            kern = L.mi_blur_last_kernel().decode()
            rx, ry = (k.rx, k.ry) if k is not None else (1, 1)
            tbs = nbytes / (us * 1e-6) / 1e12
            print(f"{name:16s} {kname:30s} {rx:3d} {ry:3d} {reps:8d} {us:10.1f} {tbs:6.2f}  {kern}", flush=True)
            rows.append({"shape": name, "kernel": kname, "rx": rx, "ry": ry, "launches": reps, "total_ms": round(ms, 1),
                         "us_per_launch": round(us, 2), "tb_s": round(tbs, 3), "kernel_name": kern,
                         "taps_x": k.taps()[0] if k is not None else [1, 2, 1]})
        del d_in, d_out
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
