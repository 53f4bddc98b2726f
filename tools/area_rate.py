#!/usr/bin/env python3
"""Rate of the area resize kernels (mi_blur_enqueue_area) on one GPU, beside the generic kernel on the same launch and,
at / 2 and / 4 of 1920x1080x3, beside the decimation presets on the same buffers: the yardsticks.

    python tools/area_rate.py [--seconds 1.0] [--json FILE] [--once] [--lib PATH]

Per point the figures are taken one after the other: the launch, the generic kernel (the same launch with the output
pointer 1 byte off; where the launch itself takes the generic kernel that column repeats it), the yardstick where the
point has one, the launch again; each is calls back to back on one stream for at least --seconds between two events
(rate_common.py), reported as us per call and TB/s = (input + output bytes) / time.  Only the first figure of a point is
preceded by a clock ramp of its own.  The difference between the two figures of the launch is the spread any gap has to
exceed.  Yardsticks (mi_blur_enqueue_sep_down with a preset, same input, same output size, same traffic):
    1920x1080x3 -> 960x540   MI_BLUR_DOWN_AREA2: blur_sep_down_tiled_kernel, the truncated 2 x 2 means
    1920x1080x3 -> 480x270   MI_BLUR_DOWN_AREA4: blur_sep_down_generic_kernel, the truncated 4 x 4 means
Points: 1920x1080x3 -> 960x540, 480x270 and 500x281 (rows of 1500 bytes: generic), 3840x2160x3 -> 1280x720,
4096x4096x1 -> 1000x1000 (rows of 1000 bytes: generic), 35 x 256x256x3 -> 128x128.
--once: five launches of each kernel per point, in order, and nothing else (for a kernel trace or a counter run).
"""
import ctypes as C

from rate_common import once, rate, save, setup

# name, images, H, W, C, Wo, Ho, preset of the yardstick (or None)
POINTS = [("1920x1080x3 -> 960x540", 1, 1080, 1920, 3, 960, 540, "AREA2"), ("1920x1080x3 -> 480x270", 1, 1080, 1920, 3, 480, 270, "AREA4"),
          ("1920x1080x3 -> 500x281", 1, 1080, 1920, 3, 500, 281, None), ("3840x2160x3 -> 1280x720", 1, 2160, 3840, 3, 1280, 720, None),
          ("4096x4096x1 -> 1000x1000", 1, 4096, 4096, 1, 1000, 1000, None), ("256x256x3 x35 -> 128x128", 35, 256, 256, 3, 128, 128, None)]


def main():
    args, torch, pkg, L = setup()
    rows = []
    print(f"{torch.cuda.get_device_name(0)}; >= {args.seconds:.1f} s of back-to-back calls per figure, after one ramp of the same length per point")
    print(f"{'point':26s} | {'us':>9s} {'again':>9s} {'TB/s':>5s} {'spread':>7s} | {'generic us':>10s} {'x':>6s} | {'yardstick us':>12s} {'launch/yard':>11s}  kernel (yardstick's)")
    for name, n, h, w, c, wo, ho, preset in POINTS:
        in_bytes, out_bytes = n * h * w * c, n * ho * wo * c
        d_in = torch.randint(0, 256, (in_bytes,), dtype=torch.uint8, device="cuda")
        d_out = torch.empty((out_bytes + 16,), dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream()
        r = pkg.Area(wo, ho)
        k, d = pkg.SepKernel(), pkg.Decimation()
        if preset:
            pkg.check(L.mi_blur_sep_down_preset(getattr(pkg, "DOWN_" + preset), C.byref(k), C.byref(d)), preset)
            assert pkg.decimated_size(w, h, d.sx, d.sy, d.ox, d.oy) == (wo, ho)

        def launch():
            pkg.check(L.mi_blur_enqueue_area(d_in.data_ptr(), d_out.data_ptr(), w, h, c, n, C.byref(r), s.cuda_stream), name)

        def generic():
            pkg.check(L.mi_blur_enqueue_area(d_in.data_ptr(), d_out.data_ptr() + 1, w, h, c, n, C.byref(r), s.cuda_stream), name)

        def yard():
            pkg.check(L.mi_blur_enqueue_sep_down(d_in.data_ptr(), d_out.data_ptr(), w, h, c, n, C.byref(k), C.byref(d), s.cuda_stream), name)

        if args.once:
            once(torch, launch, generic, *([yard] if preset else []))
            continue
        us, reps = rate(torch, launch, args.seconds, True)
        kernel = L.mi_blur_last_kernel().decode()
        gen_us, _ = rate(torch, generic, args.seconds, False)
        assert L.mi_blur_last_kernel().decode() == "blur_area_generic_kernel"
        yard_us, yard_kernel = None, ""
        if preset:
            yard_us, _ = rate(torch, yard, args.seconds, False)
            yard_kernel = L.mi_blur_last_kernel().decode()
        again, _ = rate(torch, launch, args.seconds, False)
        base = 0.5 * (us + again)
        spread = abs(us - again) / base
        tb = (in_bytes + out_bytes) / (base * 1e-6) / 1e12
        ytxt = f"{yard_us:12.1f} {base / yard_us:11.3f}" if preset else f"{'':12s} {'':11s}"
        print(f"{name:26s} | {us:9.1f} {again:9.1f} {tb:5.2f} {100 * spread:6.2f}% | {gen_us:10.1f} {gen_us / base:6.2f} | {ytxt}  {kernel} {yard_kernel}", flush=True)
        rows.append({"point": name, "launches": reps, "us": round(us, 2), "us_again": round(again, 2), "spread": round(spread, 4), "tb_s": round(tb, 3),
                     "generic_us": round(gen_us, 2), "generic_over_launch": round(gen_us / base, 3), "kernel": kernel,
                     "yardstick": preset, "yardstick_us": None if yard_us is None else round(yard_us, 2),
                     "launch_over_yardstick": None if yard_us is None else round(base / yard_us, 3), "yardstick_kernel": yard_kernel})
        del d_in, d_out
        torch.cuda.empty_cache()
    save(args, rows)


if __name__ == "__main__":
    main()
