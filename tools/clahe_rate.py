#!/usr/bin/env python3
"""Rate of the CLAHE kernels on one GPU (mi_blur_enqueue_clahe_tables, mi_blur_enqueue_clahe_apply, mi_blur_enqueue_clahe),
beside their generic kernels on the same buffers and beside the global tone call on the same input: the whole
mi_blur_enqueue_tone EQUALIZE call and its mi_blur_enqueue_hist step, code this family does not touch.

    python tools/clahe_rate.py [--seconds 1.0] [--json FILE] [--once] [--lib PATH]

Per point the input is filled two ways: the hosts' synthetic stream (mi_blur_fill_synthetic) and one constant value (a
tile of sky: every lane of a wave adds to the same counter).  Per point, data and grid the figures are taken one after the
other, each as calls back to back on one stream for at least --seconds between two events (rate_common.py), us per call:
  tables: the launch, the generic kernel (the input pointer 1 byte off), the yardstick (mi_blur_enqueue_hist on the same
          input), the launch again; TB/s = input bytes / time.
  apply:  the launch on the tables just made, the generic kernel (the output pointer 1 byte off), the yardstick (the whole
          mi_blur_enqueue_tone EQUALIZE call), the launch again; TB/s = (input + output) / time.
  clahe:  mi_blur_enqueue_clahe (both dispatches), the same with both pointers 1 byte off, the same yardstick, again.
Only the first figure of a point is preceded by a clock ramp of its own.  The difference between the two figures of a
launch is the spread any gap has to exceed.
--once: five launches of each per point, in order, and nothing else (for a kernel trace or a counter run).
"""
import ctypes as C

import numpy as np

from rate_common import once, rate, save, setup

# name, images, H, W, C
POINTS = [("1920x1080x3", 1, 1080, 1920, 3), ("4096x4096x1", 1, 4096, 4096, 1), ("4096x4096x4", 1, 4096, 4096, 4), ("256x256x3 x35", 35, 256, 256, 3)]
DATA = ("synthetic", "constant")
GRIDS = ((8, 8), (16, 16))
CLIP_Q8 = 512                                           # clip_limit 2.0


def fill(torch, L, kind, n, h, w, c):
    size = n * h * w * c
    d = torch.empty((size + 16,), dtype=torch.uint8, device="cuda")
    if kind == "synthetic":
        host = np.empty(size, np.uint8)
        L.mi_blur_fill_synthetic(host.ctypes.data, w, h, c, 0, n, 0)
        d[:size] = torch.from_numpy(host).cuda()
    else:
        d[:] = 113
    return d


def main():
    args, torch, pkg, L = setup()
    rows = []
    print(f"{torch.cuda.get_device_name(0)}; >= {args.seconds:.1f} s of back-to-back calls per figure, after one ramp of the same length per point and data")
    print(f"{'point':14s} {'data':9s} {'grid':5s} {'what':6s} | {'us':>8s} {'again':>8s} {'TB/s':>5s} {'spread':>7s} | {'generic us':>10s} {'x':>6s} | "
          f"{'yard us':>8s} {'launch/yard':>11s}  kernel (yardstick)")
    for name, n, h, w, c in POINTS:
        size = n * h * w * c
        d_hist = torch.empty((n * c * 256,), dtype=torch.int32, device="cuda")
        d_tone = torch.empty((int(L.mi_blur_tone_work_bytes(c, n)),), dtype=torch.uint8, device="cuda")
        d_out = torch.empty((size + 16,), dtype=torch.uint8, device="cuda")
        tone = pkg.Tone(pkg.TONE_EQUALIZE, 0, 0, 0, 0)
        s = torch.cuda.current_stream()
        for kind in DATA:
            d_in = fill(torch, L, kind, n, h, w, c)
            i, o = d_in.data_ptr(), d_out.data_ptr()
            ramp = True
            for grid in GRIDS:
                k = pkg.Clahe(grid[0], grid[1], CLIP_Q8, 0)
                work_bytes = int(L.mi_blur_clahe_work_bytes(w, h, c, n, C.byref(k)))
                d_work = torch.empty((work_bytes,), dtype=torch.uint8, device="cuda")
                wk = d_work.data_ptr()
                tabs_at = wk + work_bytes // 5 * 4

                def launch(call, *a):
                    return lambda: pkg.check(call(*a, s.cuda_stream), name)

                tables = launch(L.mi_blur_enqueue_clahe_tables, i, w, h, c, n, C.byref(k), wk)
                tables_generic = launch(L.mi_blur_enqueue_clahe_tables, i + 1, w, h, c, n, C.byref(k), wk)
                apply_ = launch(L.mi_blur_enqueue_clahe_apply, i, o, w, h, c, n, C.byref(k), tabs_at)
                apply_generic = launch(L.mi_blur_enqueue_clahe_apply, i, o + 1, w, h, c, n, C.byref(k), tabs_at)
                whole = launch(L.mi_blur_enqueue_clahe, i, o, w, h, c, n, C.byref(k), wk)
                whole_generic = launch(L.mi_blur_enqueue_clahe, i + 1, o + 1, w, h, c, n, C.byref(k), wk)
                yard_hist = launch(L.mi_blur_enqueue_hist, i, d_hist.data_ptr(), w, h, c, n)
                yard_tone = launch(L.mi_blur_enqueue_tone, i, o, w, h, c, n, C.byref(tone), d_tone.data_ptr())
                if args.once:
                    once(torch, tables, tables_generic, apply_, apply_generic, whole, yard_hist, yard_tone)
                    continue

                def figure(what, go, generic, yard, yard_name, moved, ramp):
                    us, reps = rate(torch, go, args.seconds, ramp)
                    kernel = L.mi_blur_last_kernel().decode()
                    gen_us = rate(torch, generic, args.seconds, False)[0]
                    gen_kernel = L.mi_blur_last_kernel().decode()
                    yard_us = rate(torch, yard, args.seconds, False)[0]
                    again = rate(torch, go, args.seconds, False)[0]
                    base = 0.5 * (us + again)
                    spread = abs(us - again) / base
                    tb = moved / (base * 1e-6) / 1e12
                    print(f"{name:14s} {kind:9s} {grid[0]:2d}x{grid[1]:<2d} {what:6s} | {us:8.1f} {again:8.1f} {tb:5.2f} {100 * spread:6.2f}% | "
                          f"{gen_us:10.1f} {gen_us / base:6.2f} | {yard_us:8.1f} {base / yard_us:11.3f}  {kernel} ({yard_name})", flush=True)
                    assert "tiled" in kernel and "generic" in gen_kernel
                    rows.append({"point": name, "data": kind, "grid": list(grid), "what": what, "launches": reps, "us": round(us, 2),
                                 "us_again": round(again, 2), "spread": round(spread, 4), "tb_s": round(tb, 3), "generic_us": round(gen_us, 2),
                                 "generic_over_launch": round(gen_us / base, 3), "kernel": kernel, "yardstick": yard_name,
                                 "yard_us": round(yard_us, 2), "launch_over_yard": round(base / yard_us, 3)})

                figure("tables", tables, tables_generic, yard_hist, "hist", size, ramp)
                figure("apply", apply_, apply_generic, yard_tone, "tone", 2 * size, False)
                figure("clahe", whole, whole_generic, yard_tone, "tone", 2 * size, False)
                ramp = False
                del d_work
            del d_in
            torch.cuda.empty_cache()
    save(args, rows)


if __name__ == "__main__":
    main()
