"""Times template matching on device 0 for profiles/r26_match.md: blur_match_tiled_kernel against blur_match_generic_kernel
on the same buffers ("match_tiled" 1 | 0), the 15 x 15 filter2d launch (mi_blur_enqueue_conv) on the same image, a ZNCC call
with its parts, and the peak search against the histogram launch on a table of the same bytes.  Every figure is the median
of `--reps` launches timed by events on the stream after `--warm` untimed ones; one line per figure.

    python tools/match_bench.py [--reps 20] [--warm 5] [--quick]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as G  # noqa: E402

pkg = G.load_package()
L = pkg.lib()


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="skip the generic kernel on the large templates (seconds a launch)")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    s = torch.cuda.current_stream().cuda_stream
    shapes = [((1, 1080, 1920, 3), t) for t in (8, 15, 32, 64)] + [((1, 4096, 4096, 1), 32), ((35, 256, 256, 3), 16)]
    images = {}
    for shape, side in shapes:
        if shape not in images:
            images[shape] = dev(rng.integers(0, 256, shape, dtype=np.uint8))
        d_in = images[shape]
        n, h, w, c = shape
        d_t = dev(rng.integers(0, 256, (side, side, c), dtype=np.uint8))
        wo, ho = w - side + 1, h - side + 1
        d_out = torch.zeros(n * wo * ho, dtype=torch.int32, device="cuda")
        macs = n * wo * ho * side * side * c
        for name in ("ccorr", "sqdiff", "sad", "zncc"):
            k = pkg.Match(pkg.MATCH_METHODS[name], side, side, 1)
            d_work = torch.zeros(L.mi_blur_match_work_bytes(w, h, c, n, C.byref(k)), dtype=torch.uint8, device="cuda")
            call = lambda: pkg.check(L.mi_blur_enqueue_match(d_in.data_ptr(), d_t.data_ptr(), d_out.data_ptr(), w, h, c, n, C.byref(k), d_work.data_ptr(), s))
            row = {}
            for tiled in (1, 0):
                if not tiled and a.quick and side > 16:
                    continue
                L.mi_blur_set_option(b"match_tiled", tiled)
                try:
                    row[tiled] = timed(call, a.reps if tiled else max(3, a.reps // 4), a.warm if tiled else 1)
                finally:
                    L.mi_blur_set_option(b"match_tiled", 1)
            line = f"{name:6s} {w}x{h}x{c} n={n} t={side}x{side}: tiled {row[1]:9.3f} ms  {macs / row[1] * 1e-9:8.2f} T byte-MAC/s"
            if 0 in row:
                line += f"  generic {row[0]:9.3f} ms  x{row[0] / row[1]:.2f}"
            print(line, flush=True)
        if side == 15:                                                  # the same byte-MACs per image as filter2d 15 x 15
            conv = pkg.Conv.from_taps(rng.integers(-8, 9, (15, 15)), shift=6)
            d_o8 = torch.zeros(n * h * w * c, dtype=torch.uint8, device="cuda")
            ms = timed(lambda: pkg.check(L.mi_blur_enqueue_conv(d_in.data_ptr(), d_o8.data_ptr(), w, h, c, n, C.byref(conv), s)), a.reps, a.warm)
            print(f"filter2d 15x15 {w}x{h}x{c}: {ms:9.3f} ms  {n * w * h * c * 225 / ms * 1e-9:8.2f} T byte-MAC/s  ({pkg.last_kernel() if hasattr(pkg, 'last_kernel') else ''})", flush=True)
        if shape == (1, 1080, 1920, 3) and side == 32:                  # the parts of the ZNCC call
            S = torch.zeros(n * h * w * c, dtype=torch.int32, device="cuda")
            Q = torch.zeros_like(S)
            iw = torch.zeros(L.mi_blur_integral_work_bytes(w, h, c, n, 1), dtype=torch.uint8, device="cuda")
            ms = timed(lambda: pkg.check(L.mi_blur_enqueue_integral(d_in.data_ptr(), S.data_ptr(), Q.data_ptr(), w, h, c, n, iw.data_ptr(), s)), a.reps, a.warm)
            print(f"  part: integral S and Q {ms:9.3f} ms", flush=True)
            table = torch.randint(0, 1 << 30, (n * ho * wo,), dtype=torch.int32, device="cuda")
            peaks = torch.zeros(n * 6, dtype=torch.int64, device="cuda")
            pw = torch.zeros(L.mi_blur_match_peak_work_bytes(wo, ho, n), dtype=torch.uint8, device="cuda")
            ms = timed(lambda: pkg.check(L.mi_blur_enqueue_match_peak(table.data_ptr(), 1, wo, ho, n, peaks.data_ptr(), pw.data_ptr(), s)), a.reps, a.warm)
            print(f"peak search {wo}x{ho} ({table.numel() * 4 / 1e6:.1f} MB): {ms:9.3f} ms  {table.numel() * 4 / ms * 1e-6:8.1f} GB/s", flush=True)
            hw = table.numel() * 4 // (h * c)                           # a byte image of the table's bytes: h rows of hw pixels
            hist = torch.zeros(c * 256, dtype=torch.int32, device="cuda")
            ms = timed(lambda: pkg.check(L.mi_blur_enqueue_hist(table.data_ptr(), hist.data_ptr(), hw, h, c, 1, s)), a.reps, a.warm)
            print(f"histogram of {hw}x{h}x{c} bytes ({hw * h * c / 1e6:.1f} MB): {ms:9.3f} ms  {hw * h * c / ms * 1e-6:8.1f} GB/s", flush=True)


if __name__ == "__main__":
    main()
