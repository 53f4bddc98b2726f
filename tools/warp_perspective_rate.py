#!/usr/bin/env python3
"""Rate of the perspective warp kernels (mi_blur_enqueue_warp_perspective, bilinear) on one GPU, beside the generic
kernel on the same launch and beside the affine tiled kernel (mi_blur_enqueue_warp) on the same images at the nearest
affine map, a rotation by 30 degrees about the centre at the same size.

    python tools/warp_perspective_rate.py [--seconds 1.0] [--json FILE] [--once] [--lib PATH]

Per point the figures are taken one after the other: the launch, the generic kernel (the same launch with an input
pointer 1 byte off), the affine launch, the launch again; each is calls back to back on one stream for at least
--seconds between two events (rate_common.py), reported as us per call and TB/s = (input + output bytes) / time.  Only
the first is preceded by a clock ramp of its own.  The difference between the two figures of the launch is the spread
any gap has to exceed.  The maps are source quads (top-left, top-right, bottom-right, bottom-left) onto the corners of
an output of the input's size, CONSTANT border:
    keystone  (0.2W, 0.1H) (0.8W, 0.1H) (W-1, H-1) (0, H-1)
    tilt      (0.1W, 0.3H) (0.9W, 0.05H) (0.95W, 0.9H) (0.3W, 0.8H)
Points: 1920x1080x3 keystone, 4096x4096x1 tilt, 35 x 256x256x3 keystone.
--once: five launches of each kernel per point, in order, and nothing else (for a kernel trace or a counter run).
"""
import ctypes as C

from rate_common import once, rate, save, setup


def quad(name, w, h):
    W, H = float(w), float(h)
    return {"keystone": [(0.2 * W, 0.1 * H), (0.8 * W, 0.1 * H), (W - 1, H - 1), (0.0, H - 1)],
            "tilt": [(0.1 * W, 0.3 * H), (0.9 * W, 0.05 * H), (0.95 * W, 0.9 * H), (0.3 * W, 0.8 * H)]}[name]


# name, images, H, W, C, quad
POINTS = [("1920x1080x3 keystone", 1, 1080, 1920, 3, "keystone"), ("4096x4096x1 tilt", 1, 4096, 4096, 1, "tilt"),
          ("256x256x3 x35 keystone", 35, 256, 256, 3, "keystone")]


def main():
    args, torch, pkg, L = setup()
    rows = []
    print(f"{torch.cuda.get_device_name(0)}; >= {args.seconds:.1f} s of back-to-back calls per figure, after one ramp of the same length per point")
    print(f"{'point':26s} | {'us':>9s} {'again':>9s} {'TB/s':>5s} {'spread':>7s} | {'generic us':>10s} {'x':>6s} | {'affine us':>9s} {'TB/s':>5s} {'persp/affine':>12s}  kernel")
    for name, n, h, w, c, qname in POINTS:
        in_bytes = out_bytes = n * h * w * c
        d_in = torch.randint(0, 256, (in_bytes + 16,), dtype=torch.uint8, device="cuda")
        d_off = torch.empty_like(d_in)
        d_off[1:1 + in_bytes] = d_in[:in_bytes]           # the same images, 1 byte into their buffer
        d_out = torch.empty((out_bytes,), dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream()
        corners = [(0.0, 0.0), (w - 1.0, 0.0), (w - 1.0, h - 1.0), (0.0, h - 1.0)]
        pp = pkg.WarpPerspective.from_matrix(pkg.perspective_matrix(quad(qname, w, h), corners), w, h, "bilinear", "constant", 0)
        wp = pkg.Warp.from_matrix(pkg.rotation_matrix(((w - 1) / 2, (h - 1) / 2), 30.0), w, h, "bilinear", "constant", 0)

        def launch():
            pkg.check(L.mi_blur_enqueue_warp_perspective(d_in.data_ptr(), d_out.data_ptr(), w, h, c, n, C.byref(pp), s.cuda_stream), name)

        def generic():
            pkg.check(L.mi_blur_enqueue_warp_perspective(d_off.data_ptr() + 1, d_out.data_ptr(), w, h, c, n, C.byref(pp), s.cuda_stream), name)

        def affine():
            pkg.check(L.mi_blur_enqueue_warp(d_in.data_ptr(), d_out.data_ptr(), w, h, c, n, C.byref(wp), s.cuda_stream), name)

        if args.once:
            once(torch, launch, generic, affine)
            continue
        us, reps = rate(torch, launch, args.seconds, True)
        kernel = L.mi_blur_last_kernel().decode()
        gen_us, _ = rate(torch, generic, args.seconds, False)
        assert L.mi_blur_last_kernel().decode() == "blur_warp_persp_generic_kernel"
        aff_us, _ = rate(torch, affine, args.seconds, False)
        assert L.mi_blur_last_kernel().decode() == "blur_warp_tiled_kernel"
        again, _ = rate(torch, launch, args.seconds, False)
        base = 0.5 * (us + again)
        spread = abs(us - again) / base
        moved = in_bytes + out_bytes
        tb, aff_tb = moved / (base * 1e-6) / 1e12, moved / (aff_us * 1e-6) / 1e12
        print(f"{name:26s} | {us:9.1f} {again:9.1f} {tb:5.2f} {100 * spread:6.2f}% | {gen_us:10.1f} {gen_us / base:6.2f} | {aff_us:9.1f} {aff_tb:5.2f} {base / aff_us:12.2f}  {kernel}", flush=True)
        rows.append({"point": name, "launches": reps, "us": round(us, 2), "us_again": round(again, 2), "spread": round(spread, 4), "tb_s": round(tb, 3),
                     "generic_us": round(gen_us, 2), "generic_over_launch": round(gen_us / base, 3), "affine_us": round(aff_us, 2),
                     "affine_tb_s": round(aff_tb, 3), "launch_over_affine": round(base / aff_us, 3), "kernel": kernel})
        del d_in, d_off, d_out
        torch.cuda.empty_cache()
    save(args, rows)


if __name__ == "__main__":
    main()
