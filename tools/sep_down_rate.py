#!/usr/bin/env python3
"""Rate of the decimating separable kernel (mi_blur_enqueue_sep_down) on one GPU, beside what a caller had to launch
before it existed: mi_blur_enqueue_sep with the same taps on the same input (and then subsample).

    python tools/sep_down_rate.py [--seconds 1.0] [--json FILE] [--once] [--lib PATH]

Per point three figures are taken one after the other: the baseline, the decimating launch, the baseline again; each
is launches back to back on one stream for at least --seconds between two events, reported as us per launch and
TB/s = (input + output bytes) / time.  Only the first is preceded by a clock ramp of its own (--seconds of launches
that are not counted); the other two follow a one-second run directly and rely on it.  The difference between the two
baseline figures is the spread any gap has to exceed.  floor_tb_s (8192x8192x3 at stride 2 only) is the 252 MB such a
launch has to move at least, over the measured time: compare it with the measured copy ceiling (tools/copy_ceiling.py,
~6.29 TB/s), not with a data-sheet peak.  Shapes: one 8192x8192x3 image, and a batch of 8 1920x1080x3 frames.  Kernels: MI_BLUR_DOWN_PYR, Gaussian
sigma 1 and 2 at stride 2, MI_BLUR_DOWN_AREA2.  --once: five launches of each per point, in order, and nothing else (for a kernel trace).
--lib PATH: time that build of libmi_blur.so instead of the tree's (rate_common.py).
"""
import ctypes as C

from rate_common import once, rate, save, setup

SHAPES = [("8192x8192x3", 1, 8192, 8192, 3), ("1920x1080x3 x8", 8, 1080, 1920, 3)]
HBM_FLOOR_8192 = 252e6        # bytes one 8192x8192x3 launch at stride 2 has to move: 201.3 MB in + 50.3 MB out


def main():
    args, torch, pkg, L = setup()

    def preset(which):
        k, d = pkg.SepKernel(), pkg.Decimation()
        pkg.check(L.mi_blur_sep_down_preset(which, C.byref(k), C.byref(d)), "mi_blur_sep_down_preset")
        return k, d

    two = pkg.Decimation(2, 2, 0, 0)
    kernels = [("MI_BLUR_DOWN_PYR", *preset(pkg.DOWN_PYR)), ("gauss sigma 1, stride 2", pkg.gauss_kernel(1.0), two),
               ("gauss sigma 2, stride 2", pkg.gauss_kernel(2.0), two), ("MI_BLUR_DOWN_AREA2", *preset(pkg.DOWN_AREA2))]
    rows = []
    print(f"{torch.cuda.get_device_name(0)}; >= {args.seconds:.1f} s of back-to-back launches per figure, after a ramp of the same length")
    print(f"{'shape':16s} {'kernel':24s} {'rx':>3s} | {'sep us':>9s} {'again':>9s} {'TB/s':>5s} | {'down us':>9s} {'TB/s':>5s} | {'down/sep':>8s} {'spread':>7s}  kernels")
    for name, n, h, w, c in SHAPES:
        d_in = torch.randint(0, 256, (n, h, w, c), dtype=torch.uint8, device="cuda")
        d_full = torch.empty_like(d_in)
        s = torch.cuda.current_stream()
        for kname, k, d in kernels:
            wo, ho = pkg.decimated_size(w, h, d.sx, d.sy, d.ox, d.oy)
            d_down = torch.empty((n, ho, wo, c), dtype=torch.uint8, device="cuda")

            def sep():
                pkg.check(L.mi_blur_enqueue_sep(d_in.data_ptr(), d_full.data_ptr(), w, h, c, n, C.byref(k), s.cuda_stream), kname)

            def down():
                pkg.check(L.mi_blur_enqueue_sep_down(d_in.data_ptr(), d_down.data_ptr(), w, h, c, n, C.byref(k), C.byref(d), s.cuda_stream), kname)

            if args.once:                            # 5 + 5 dispatches per point, in this order
                once(torch, sep, down)
                continue

            def timed(go, ramp=False):
                return (*rate(torch, go, args.seconds, ramp, warm=3, probe=10, min_reps=20), L.mi_blur_last_kernel().decode())

            sep_us, _, sep_kernel = timed(sep, True)
            down_us, reps, down_kernel = timed(down)
            sep_again, _, _ = timed(sep)
            sep_bytes, down_bytes = 2 * d_in.numel(), d_in.numel() + d_down.numel()
            base = 0.5 * (sep_us + sep_again)
            spread = abs(sep_us - sep_again) / base
            ratio = down_us / base
            print(f"{name:16s} {kname:24s} {k.rx:3d} | {sep_us:9.1f} {sep_again:9.1f} {sep_bytes / (base * 1e-6) / 1e12:5.2f} | "
                  f"{down_us:9.1f} {down_bytes / (down_us * 1e-6) / 1e12:5.2f} | {ratio:8.3f} {100 * spread:6.2f}%  {sep_kernel} / {down_kernel}", flush=True)
            row = {"shape": name, "kernel": kname, "rx": k.rx, "ry": k.ry, "launches": reps, "sep_us": round(sep_us, 2), "sep_us_again": round(sep_again, 2),
                   "down_us": round(down_us, 2), "down_over_sep": round(ratio, 4), "baseline_spread": round(spread, 4),
                   "sep_tb_s": round(sep_bytes / (base * 1e-6) / 1e12, 3), "down_tb_s": round(down_bytes / (down_us * 1e-6) / 1e12, 3),
                   "sep_kernel": sep_kernel, "down_kernel": down_kernel}
            if n == 1 and (d.sx, d.sy) == (2, 2):
                row["floor_tb_s"] = round(HBM_FLOOR_8192 / (down_us * 1e-6) / 1e12, 3)      # the bytes it must move / the time it took
            rows.append(row)
            del d_down
        del d_in, d_full
        torch.cuda.empty_cache()
    save(args, rows)


if __name__ == "__main__":
    main()
