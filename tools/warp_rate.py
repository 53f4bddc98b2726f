#!/usr/bin/env python3
"""Rate of the affine warp kernels (mi_blur_enqueue_warp, bilinear) on one GPU, beside a device-to-device copy of the
same number of bytes in the same run (the method of tools/copy_ceiling.py: torch's copy_ of an int32 view, which reads
N and writes N bytes; here N = (input + output bytes) / 2) and beside the generic kernel on the same launch.

    python tools/warp_rate.py [--seconds 1.0] [--json FILE] [--once] [--lib PATH]

Per point the figures are taken one after the other: the launch, the copy, the generic kernel, the launch again; each
is calls back to back on one stream for at least --seconds between two events, reported as us per call and
TB/s = (input + output bytes) / time.  Only the first is preceded by a clock ramp of its own (--seconds of launches that
are not counted).  The difference between the two figures of the launch is the spread any gap has to exceed.  The
generic kernel is reached by handing the same launch an input pointer that is 1 byte off (its reads are single bytes, so
the misalignment costs it nothing); where the launch itself takes the generic kernel that column repeats it.
Points: 8 x 1920x1080x3 and 8192x8192x3 rotated 30 degrees about the centre at the same size (CONSTANT border),
8 x 1920x1080x4 rotated 45 degrees, and 1920x1080x3 under the x2 CLAMP warp, which gives the bytes of the x2 resize:
that point also times blur_resize_tiled_kernel on the same images (the last column, after the generic kernel).
--once: five launches of each kernel per point, in order, and nothing else (for a kernel trace).  --lib PATH: time that
build of libmi_blur.so instead of the tree's (rate_common.py).
"""
import ctypes as C

from rate_common import once, rate, save, setup

Q = 1 << 16
# name, images, H, W, C, Wo, Ho, rotation in degrees (None: the x2 CLAMP warp {Q/2, 0, -Q/4, 0, Q/2, -Q/4})
POINTS = [("1920x1080x3 x8 rotate 30", 8, 1080, 1920, 3, 1920, 1080, 30.0), ("8192x8192x3 rotate 30", 1, 8192, 8192, 3, 8192, 8192, 30.0),
          ("1920x1080x4 x8 rotate 45", 8, 1080, 1920, 4, 1920, 1080, 45.0), ("1920x1080x3 x2 clamp", 1, 1080, 1920, 3, 3840, 2160, None)]


def main():
    args, torch, pkg, L = setup()
    rows = []
    print(f"{torch.cuda.get_device_name(0)}; >= {args.seconds:.1f} s of back-to-back calls per figure, after one ramp of the same length per point")
    print(f"{'point':30s} | {'us':>9s} {'again':>9s} {'TB/s':>5s} {'spread':>7s} | {'copy us':>9s} {'TB/s':>5s} {'of copy':>7s} | {'generic us':>10s} {'x':>6s} | {'resize us':>9s} {'x':>6s}  kernel")
    for name, n, h, w, c, wo, ho, angle in POINTS:
        in_bytes, out_bytes = n * h * w * c, n * ho * wo * c
        d_in = torch.randint(0, 256, (in_bytes + 16,), dtype=torch.uint8, device="cuda")
        d_off = torch.empty_like(d_in)
        d_off[1:1 + in_bytes] = d_in[:in_bytes]           # the same images, 1 byte into their buffer
        d_out = torch.empty((out_bytes,), dtype=torch.uint8, device="cuda")
        half = (in_bytes + out_bytes) // 2 // 4 * 4
        c_src = torch.randint(0, 256, (half,), dtype=torch.uint8, device="cuda").view(torch.int32)
        c_dst = torch.empty_like(c_src)
        s = torch.cuda.current_stream()
        if angle is None:
            wp = pkg.Warp(wo, ho, pkg.RESIZE_BILINEAR, pkg.WARP_CLAMP, 0, (C.c_int64 * 6)(Q // 2, 0, -Q // 4, 0, Q // 2, -Q // 4))
        else:
            wp = pkg.Warp.from_matrix(pkg.rotation_matrix(((w - 1) / 2, (h - 1) / 2), angle), wo, ho, "bilinear", "constant", 0)
        r = pkg.Resize(wo, ho, pkg.RESIZE_BILINEAR)

        def launch():
            pkg.check(L.mi_blur_enqueue_warp(d_in.data_ptr(), d_out.data_ptr(), w, h, c, n, C.byref(wp), s.cuda_stream), name)

        def generic():
            pkg.check(L.mi_blur_enqueue_warp(d_off.data_ptr() + 1, d_out.data_ptr(), w, h, c, n, C.byref(wp), s.cuda_stream), name)

        def resize():
            pkg.check(L.mi_blur_enqueue_resize(d_in.data_ptr(), d_out.data_ptr(), w, h, c, n, C.byref(r), s.cuda_stream), name)

        def copy():
            c_dst.copy_(c_src)

        if args.once:
            once(torch, launch, generic)
            continue

        def timed(go, ramp=False):
            return rate(torch, go, args.seconds, ramp)

        us, reps = timed(launch, True)
        kernel = L.mi_blur_last_kernel().decode()
        copy_us, _ = timed(copy)
        gen_us, _ = timed(generic)
        assert L.mi_blur_last_kernel().decode() == "blur_warp_generic_kernel"
        resize_us = None
        if angle is None:
            resize_us, _ = timed(resize)
            assert L.mi_blur_last_kernel().decode() == "blur_resize_tiled_kernel"
        again, _ = timed(launch)
        base = 0.5 * (us + again)
        spread = abs(us - again) / base
        moved = in_bytes + out_bytes
        tb, copy_tb = moved / (base * 1e-6) / 1e12, 2 * half / (copy_us * 1e-6) / 1e12
        print(f"{name:30s} | {us:9.1f} {again:9.1f} {tb:5.2f} {100 * spread:6.2f}% | {copy_us:9.1f} {copy_tb:5.2f} {tb / copy_tb:7.3f} | "
              f"{gen_us:10.1f} {gen_us / base:6.2f} | " + (f"{resize_us:9.1f} {resize_us / base:6.2f}" if resize_us else f"{'-':>9s} {'-':>6s}") + f"  {kernel}", flush=True)
        rows.append({"point": name, "launches": reps, "us": round(us, 2), "us_again": round(again, 2), "spread": round(spread, 4),
                     "tb_s": round(tb, 3), "copy_us": round(copy_us, 2), "copy_tb_s": round(copy_tb, 3), "fraction_of_copy": round(tb / copy_tb, 4),
                     "generic_us": round(gen_us, 2), "generic_over_launch": round(gen_us / base, 3),
                     "resize_us": resize_us and round(resize_us, 2), "resize_over_launch": resize_us and round(resize_us / base, 3), "kernel": kernel})
        del d_in, d_off, d_out, c_src, c_dst
        torch.cuda.empty_cache()
    save(args, rows)


if __name__ == "__main__":
    main()
