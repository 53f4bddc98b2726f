#!/usr/bin/env python3
"""Rate of the histogram family's kernels on one GPU (mi_blur_enqueue_hist, mi_blur_enqueue_tables, mi_blur_enqueue_tone),
beside their generic kernels on the same buffers and beside the colour transform on the same input: code this family
does not touch, which reads the same bytes.

    python tools/hist_rate.py [--seconds 1.0] [--json FILE] [--once] [--lib PATH]

Per point the input is filled three ways: uniform random bytes, the hosts' synthetic stream (mi_blur_fill_synthetic) and
one constant value, the hard case of a histogram: every lane of a wave adds to the same counter.  Per point and data
the figures are taken one after the other, each as calls back to back on one stream for at least --seconds between two
events (rate_common.py), us per call:
  hist:   the launch (zeroing + blur_hist_tiled_kernel), the generic kernel (the input pointer 1 byte off), the yardstick
          (mi_blur_enqueue_color C -> 1 on the same input), the launch again; TB/s = input bytes / time.
  tables: mi_blur_enqueue_tables (a permutation per image and channel), its generic kernel (the output pointer 1 byte
          off), the yardstick (mi_blur_enqueue_color C -> C, the identity matrix with a table), the launch again; then
  tone:   mi_blur_enqueue_tone (three dispatches), twice, against the same yardstick; TB/s = (input + output) / time.
Only the first figure of a point is preceded by a clock ramp of its own.  The difference between the two figures of a
launch is the spread any gap has to exceed.
--once: five launches of each per point, in order, and nothing else (for a kernel trace or a counter run).
"""
import ctypes as C

import numpy as np

from rate_common import once, rate, save, setup

# name, images, H, W, C
POINTS = [("1920x1080x3", 1, 1080, 1920, 3), ("4096x4096x1", 1, 4096, 4096, 1), ("4096x4096x4", 1, 4096, 4096, 4), ("256x256x3 x35", 35, 256, 256, 3)]
DATA = ("random", "synthetic", "constant")


def fill(torch, L, kind, n, h, w, c):
    size = n * h * w * c
    d = torch.empty((size + 16,), dtype=torch.uint8, device="cuda")
    if kind == "random":
        d[:size] = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda")
    elif kind == "synthetic":
        host = np.empty(size, np.uint8)
        L.mi_blur_fill_synthetic(host.ctypes.data, w, h, c, 0, n, 0)
        d[:size] = torch.from_numpy(host).cuda()
    else:
        d[:] = 113
    return d


def main():
    args, torch, pkg, L = setup()
    rows = []
    rng = np.random.default_rng(1)
    print(f"{torch.cuda.get_device_name(0)}; >= {args.seconds:.1f} s of back-to-back calls per figure, after one ramp of the same length per point and data")
    head = f"{'point':14s} {'data':9s} {'what':6s} | {'us':>8s} {'again':>8s} {'TB/s':>5s} {'spread':>7s} | {'generic us':>10s} {'x':>6s} | {'colour us':>9s} {'launch/colour':>13s}  kernel"
    print(head)
    for name, n, h, w, c in POINTS:
        size = n * h * w * c
        to_one, ident = pkg.Color(), pkg.Color()
        to_one.out_channels, to_one.m[0][0] = 1, 1
        pkg.check(L.mi_blur_color_identity(c, C.byref(ident)), "mi_blur_color_identity")
        tables = np.stack([rng.permutation(256) for _ in range(n * c)]).astype(np.uint8)
        for o in range(c):
            C.memmove(ident.lut[o], tables[o].ctypes.data, 256)
        ident.lut_on = 1
        d_tab = torch.from_numpy(tables.reshape(-1)).cuda()
        d_hist = torch.empty((n * c * 256,), dtype=torch.int32, device="cuda")
        d_work = torch.empty((int(L.mi_blur_tone_work_bytes(c, n)),), dtype=torch.uint8, device="cuda")
        d_out = torch.empty((size + 16,), dtype=torch.uint8, device="cuda")
        tone = pkg.Tone(pkg.TONE_EQUALIZE, 0, 0, 0, 0)
        s = torch.cuda.current_stream()
        for kind in DATA:
            d_in = fill(torch, L, kind, n, h, w, c)
            i, o = d_in.data_ptr(), d_out.data_ptr()

            def launch(call, *a):
                return lambda: pkg.check(call(*a, s.cuda_stream), name)

            hist = launch(L.mi_blur_enqueue_hist, i, d_hist.data_ptr(), w, h, c, n)
            hist_generic = launch(L.mi_blur_enqueue_hist, i + 1, d_hist.data_ptr(), w, h, c, n)
            yard_one = launch(L.mi_blur_enqueue_color, i, o, w, h, c, n, C.byref(to_one))
            tabs = launch(L.mi_blur_enqueue_tables, i, o, w, h, c, n, d_tab.data_ptr())
            tabs_generic = launch(L.mi_blur_enqueue_tables, i, o + 1, w, h, c, n, d_tab.data_ptr())
            yard_same = launch(L.mi_blur_enqueue_color, i, o, w, h, c, n, C.byref(ident))
            tone_go = launch(L.mi_blur_enqueue_tone, i, o, w, h, c, n, C.byref(tone), d_work.data_ptr())
            if args.once:
                once(torch, hist, hist_generic, yard_one, tabs, tabs_generic, yard_same, tone_go)
                continue

            def figure(what, go, generic, yard, moved, ramp):
                us, reps = rate(torch, go, args.seconds, ramp)
                kernel = L.mi_blur_last_kernel().decode()
                gen_us = rate(torch, generic, args.seconds, False)[0] if generic else None
                gen_kernel = L.mi_blur_last_kernel().decode()
                yard_us = rate(torch, yard, args.seconds, False)[0]
                again = rate(torch, go, args.seconds, False)[0]
                base = 0.5 * (us + again)
                spread = abs(us - again) / base
                tb = moved / (base * 1e-6) / 1e12
                gen = f"{gen_us:10.1f} {gen_us / base:6.2f}" if generic else f"{'-':>10s} {'-':>6s}"
                print(f"{name:14s} {kind:9s} {what:6s} | {us:8.1f} {again:8.1f} {tb:5.2f} {100 * spread:6.2f}% | {gen} | {yard_us:9.1f} {base / yard_us:13.3f}  {kernel}", flush=True)
                assert generic is None or "generic" in gen_kernel
                rows.append({"point": name, "data": kind, "what": what, "launches": reps, "us": round(us, 2), "us_again": round(again, 2),
                             "spread": round(spread, 4), "tb_s": round(tb, 3), "generic_us": round(gen_us, 2) if generic else None,
                             "generic_over_launch": round(gen_us / base, 3) if generic else None, "kernel": kernel,
                             "colour_us": round(yard_us, 2), "launch_over_colour": round(base / yard_us, 3)})

            figure("hist", hist, hist_generic, yard_one, size, True)
            figure("tables", tabs, tabs_generic, yard_same, 2 * size, False)
            figure("tone", tone_go, None, yard_same, 2 * size, False)
            del d_in
            torch.cuda.empty_cache()
    save(args, rows)


if __name__ == "__main__":
    main()
