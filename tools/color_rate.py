#!/usr/bin/env python3
"""Rate of the colour transform kernels (mi_blur_enqueue_color) on one GPU, beside the generic kernel on the same
buffers and beside the plain 3x3 launch on an input of the same byte count: the project's yardstick for a streaming kernel.

    python tools/color_rate.py [--seconds 1.0] [--json FILE] [--once] [--lib PATH]

Per point and per lut_on the figures are taken one after the other: the launch, the generic kernel (the same launch
with the output pointer 1 byte off), the yardstick (mi_blur_enqueue, radius 1, on the same input buffer and shape), the
launch again; each is calls back to back on one stream for at least --seconds between two events (rate_common.py),
reported as us per call and TB/s = (input + output bytes) / time: W*H*(C+Co) for the transform, 2*W*H*C for the
yardstick.  Only the first figure of a point is preceded by a clock ramp of its own.  The difference between the two
figures of the launch is the spread any gap has to exceed.  With lut_on the table is a permutation per channel.
--once: five launches of each kernel per point, in order, and nothing else (for a kernel trace or a counter run).
"""
import ctypes as C

import numpy as np

from rate_common import once, rate, save, setup

# name, images, H, W, preset
POINTS = [("1920x1080 3->1 gray", 1, 1080, 1920, "rgb2gray"), ("1920x1080 3->3 ycbcr", 1, 1080, 1920, "rgb2ycbcr"),
          ("1920x1080 3->4 rgba", 1, 1080, 1920, "rgb2rgba"), ("4096x4096 4->1 gray", 1, 4096, 4096, "rgb2gray4"),
          ("256x256 x35 3->1 gray", 35, 256, 256, "rgb2gray")]


def main():
    args, torch, pkg, L = setup()
    rows = []
    rng = np.random.default_rng(1)
    print(f"{torch.cuda.get_device_name(0)}; >= {args.seconds:.1f} s of back-to-back calls per figure, after one ramp of the same length per point")
    print(f"{'point':24s} lut | {'us':>8s} {'again':>8s} {'TB/s':>5s} {'spread':>7s} | {'generic us':>10s} {'x':>6s} | {'3x3 us':>8s} {'TB/s':>5s} {'launch/3x3':>10s}  kernel")
    for name, n, h, w, preset in POINTS:
        c = 4 if preset.endswith("4") else 3
        for lut_on in (0, 1):
            k = pkg.color_preset(preset.rstrip("4"))
            co = k.out_channels
            if lut_on:
                for o in range(co):
                    t = rng.permutation(256).astype(np.uint8)
                    C.memmove(k.lut[o], t.ctypes.data, 256)
                k.lut_on = 1
            in_bytes, out_bytes = n * h * w * c, n * h * w * co
            d_in = torch.randint(0, 256, (in_bytes,), dtype=torch.uint8, device="cuda")
            d_out = torch.empty((max(out_bytes, in_bytes) + 16,), dtype=torch.uint8, device="cuda")
            s = torch.cuda.current_stream()

            def launch():
                pkg.check(L.mi_blur_enqueue_color(d_in.data_ptr(), d_out.data_ptr(), w, h, c, n, C.byref(k), s.cuda_stream), name)

            def generic():
                pkg.check(L.mi_blur_enqueue_color(d_in.data_ptr(), d_out.data_ptr() + 1, w, h, c, n, C.byref(k), s.cuda_stream), name)

            def yard():
                pkg.check(L.mi_blur_enqueue(d_in.data_ptr(), d_out.data_ptr(), w, h, c, 1, n, s.cuda_stream), name)

            if args.once:
                once(torch, launch, generic, yard)
                continue
            us, reps = rate(torch, launch, args.seconds, True)
            kernel = L.mi_blur_last_kernel().decode()
            assert kernel == "blur_color_tiled_kernel"
            gen_us, _ = rate(torch, generic, args.seconds, False)
            assert L.mi_blur_last_kernel().decode() == "blur_color_generic_kernel"
            yard_us, _ = rate(torch, yard, args.seconds, False)
            yard_kernel = L.mi_blur_last_kernel().decode()
            again, _ = rate(torch, launch, args.seconds, False)
            base = 0.5 * (us + again)
            spread = abs(us - again) / base
            tb = (in_bytes + out_bytes) / (base * 1e-6) / 1e12
            ytb = 2 * in_bytes / (yard_us * 1e-6) / 1e12
            print(f"{name:24s} {lut_on:3d} | {us:8.1f} {again:8.1f} {tb:5.2f} {100 * spread:6.2f}% | {gen_us:10.1f} {gen_us / base:6.2f} | "
                  f"{yard_us:8.1f} {ytb:5.2f} {base / yard_us:10.3f}  {kernel} ({yard_kernel})", flush=True)
            rows.append({"point": name, "lut_on": lut_on, "launches": reps, "us": round(us, 2), "us_again": round(again, 2), "spread": round(spread, 4),
                         "tb_s": round(tb, 3), "generic_us": round(gen_us, 2), "generic_over_launch": round(gen_us / base, 3), "kernel": kernel,
                         "yardstick_us": round(yard_us, 2), "yardstick_tb_s": round(ytb, 3), "launch_over_yardstick": round(base / yard_us, 3),
                         "yardstick_kernel": yard_kernel})
            del d_in, d_out
            torch.cuda.empty_cache()
    save(args, rows)


if __name__ == "__main__":
    main()
