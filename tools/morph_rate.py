#!/usr/bin/env python3
"""Rate of the morphology kernels (mi_blur_enqueue_morph) on one GPU, beside the separable blur of the same radii
(mi_blur_enqueue_sep) and the fixed radius-1 kernel (mi_blur_enqueue), all in one run.

    python tools/morph_rate.py [--seconds 1.0] [--repeats 3] [--json FILE]

Per point: launches back to back on one stream for at least --seconds between two events (after a warm-up that also
sizes the run), --repeats times; reported as the smallest and largest us per launch and algorithmic TB/s (input + output
bytes once each, from the smallest).  Shapes: one 8192x8192x3 image, and a batch of 8 1920x1080x3 frames.  Square radii
1, 3, 6, 8, 13, 16: ERODE, DILATE, GRADIENT and a separable kernel of exactly that radius per axis (2r+1 non-zero taps
summing to 256, so that no tap is trimmed).
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
RADII = (1, 3, 6, 8, 13, 16)


def full_taps(r):
    """2r+1 non-zero taps summing to 256: ones, the centre takes the rest."""
    t = [1] * (2 * r + 1)
    t[r] = 256 - 2 * r
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    import torch
    pkg = entry.load_package()
    L = pkg.lib()
    torch.cuda.set_device(0)
    points = []
    for r in RADII:
        k = pkg.SepKernel.from_taps(full_taps(r))
        assert (k.rx, k.ry) == (r, r)
        points.append((f"sep blur r={r}", r, ("sep", k)))
        for name, op in (("erode", pkg.MORPH_ERODE), ("dilate", pkg.MORPH_DILATE), ("gradient", pkg.MORPH_GRADIENT)):
            points.append((f"{name} r={r}", r, ("morph", op)))
    points.append(("mi_blur_enqueue radius 1", 1, ("box", 1)))
    rows = []
    print(f"{torch.cuda.get_device_name(0)}; >= {args.seconds:.1f} s of back-to-back launches per point, {args.repeats} times")
    print(f"{'shape':16s} {'kernel':26s} {'r':>3s} {'launches':>8s} {'us min':>9s} {'us max':>9s} {'TB/s':>6s}  kernel name")
    for name, n, h, w, c in SHAPES:
        d_in = torch.randint(0, 256, (n, h, w, c), dtype=torch.uint8, device="cuda")
        d_out = torch.empty_like(d_in)
        s = torch.cuda.current_stream()
        nbytes = 2 * d_in.numel()
        for kname, r, (kind, arg) in points:
            def go():
                if kind == "box":
                    rc = L.mi_blur_enqueue(d_in.data_ptr(), d_out.data_ptr(), w, h, c, arg, n, s.cuda_stream)
                elif kind == "sep":
                    rc = L.mi_blur_enqueue_sep(d_in.data_ptr(), d_out.data_ptr(), w, h, c, n, C.byref(arg), s.cuda_stream)
                else:
                    rc = L.mi_blur_enqueue_morph(d_in.data_ptr(), d_out.data_ptr(), w, h, c, arg, r, r, n, s.cuda_stream)
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
            us = []
            for _ in range(args.repeats):
                e0.record()
                for _ in range(reps):
                    go()
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / reps)
            kern = L.mi_blur_last_kernel().decode()
            tbs = nbytes / (min(us) * 1e-6) / 1e12
            print(f"{name:16s} {kname:26s} {r:3d} {reps:8d} {min(us):9.1f} {max(us):9.1f} {tbs:6.2f}  {kern}", flush=True)
            rows.append({"shape": name, "kernel": kname, "r": r, "launches": reps, "us_min": round(min(us), 2),
                         "us_max": round(max(us), 2), "us_all": [round(u, 2) for u in us], "tb_s": round(tbs, 3), "kernel_name": kern})
        del d_in, d_out
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
