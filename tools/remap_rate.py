#!/usr/bin/env python3
"""Rate of the remap kernels (mi_blur_enqueue_remap, bilinear) on one GPU, beside the generic kernel on the same launch
and beside the affine tiled kernel (mi_blur_enqueue_warp) on the same images at the same rotation: the yardstick.

    python tools/remap_rate.py [--seconds 1.0] [--json FILE] [--once] [--lib PATH]

Per point and map the figures are taken one after the other: the launch, the generic kernel (the same launch with the
map pointer 8 bytes off), the affine launch (a rotation by 30 degrees about the centre at the same size), the launch
again; each is calls back to back on one stream for at least --seconds between two events (rate_common.py), reported as
us per call and TB/s = (input + output + map bytes) / time, the map's 8 bytes per output pixel counted once per launch
(one map serves every image; the affine launch moves input + output only).  Only the first figure of a point is
preceded by a clock ramp of its own.  The difference between the two figures of the launch is the spread any gap has to
exceed.  CONSTANT border, output of the input's size.  Maps:
    rot30   the affine launch's own positions: px = (Sx + 16) >> 5 of its Q16 matrix, so both sample the same places
    barrel  mi_blur_remap_undistort with fx = fy = W, the centre as principal point, dist -0.2, 0.05, 0.001, -0.002, 0.01
Points: 1920x1080x3, 4096x4096x1, 35 x 256x256x3.  Every point and map at the default stage_bytes and at "fit": the
largest box mi_blur_remap_plan finds, the smallest stage_bytes that still stages every tile (what a caller who holds the
map would pass); at 1080p rot30 also at 32752.  The plan's counts of staged, direct and empty tiles are printed beside
every figure.
--once: five launches of each kernel per point, in order, and nothing else (for a kernel trace or a counter run).
"""
import ctypes as C

import numpy as np

from rate_common import once, rate, save, setup

DIST = (-0.2, 0.05, 0.001, -0.002, 0.01)
# name, images, H, W, C
POINTS = [("1920x1080x3", 1, 1080, 1920, 3), ("4096x4096x1", 1, 4096, 4096, 1), ("256x256x3 x35", 35, 256, 256, 3)]


def rot30_map(wp, w, h):
    """The positions of the affine warp wp, rounded to 11 fraction bits as the header rounds them."""
    Y, X = np.mgrid[0:h, 0:w].astype(np.int64)
    m = list(wp.m)
    px, py = (m[0] * X + m[1] * Y + m[2] + 16) >> 5, (m[3] * X + m[4] * Y + m[5] + 16) >> 5
    return np.stack([px, py], axis=-1).clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32)


def main():
    args, torch, pkg, L = setup()
    rows = []
    print(f"{torch.cuda.get_device_name(0)}; >= {args.seconds:.1f} s of back-to-back calls per figure, after one ramp of the same length per point")
    print(f"{'point':16s} {'map':7s} {'stage':>6s} | {'us':>9s} {'again':>9s} {'TB/s':>5s} {'spread':>7s} | {'generic us':>10s} {'x':>6s} | {'affine us':>9s} {'TB/s':>5s} {'remap/affine':>12s} {'traffic':>7s} | staged direct empty  kernel")
    for name, n, h, w, c in POINTS:
        in_bytes = out_bytes = n * h * w * c
        map_bytes = h * w * 8
        d_in = torch.randint(0, 256, (in_bytes,), dtype=torch.uint8, device="cuda")
        d_out = torch.empty((out_bytes,), dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream()
        wp = pkg.Warp.from_matrix(pkg.rotation_matrix(((w - 1) / 2, (h - 1) / 2), 30.0), w, h, "bilinear", "constant", 0)
        first = True
        for mname in ("rot30", "barrel"):
            fmap = rot30_map(wp, w, h) if mname == "rot30" else pkg.undistort_map((float(w), float(w), (w - 1) / 2, (h - 1) / 2), DIST, (w, h))
            d_map = torch.zeros((map_bytes + 16,), dtype=torch.uint8, device="cuda")
            flat = torch.from_numpy(fmap.view(np.uint8).reshape(-1)).cuda()
            d_map[:map_bytes] = flat
            d_map_off = torch.zeros_like(d_map)
            d_map_off[8:8 + map_bytes] = flat                    # the same map, 8 bytes into its buffer
            # the default, then "fit": the largest box the plan found, the smallest stage_bytes that still stages every tile
            fit = max(16, pkg.remap_plan(fmap, w, h, c, "bilinear", "constant")["max_box_bytes"])
            assert fit <= 65520
            for stage in ((0, 32752, fit) if (name, mname) == ("1920x1080x3", "rot30") else (0, fit)):
                r = pkg.Remap(w, h, pkg.RESIZE_BILINEAR, pkg.WARP_CONSTANT, 0, stage)
                plan = pkg.remap_plan(fmap, w, h, c, "bilinear", "constant", 0, stage)

                def launch():
                    pkg.check(L.mi_blur_enqueue_remap(d_in.data_ptr(), d_out.data_ptr(), w, h, c, n, C.byref(r), d_map.data_ptr(), s.cuda_stream), name)

                def generic():
                    pkg.check(L.mi_blur_enqueue_remap(d_in.data_ptr(), d_out.data_ptr(), w, h, c, n, C.byref(r), d_map_off.data_ptr() + 8, s.cuda_stream), name)

                def affine():
                    pkg.check(L.mi_blur_enqueue_warp(d_in.data_ptr(), d_out.data_ptr(), w, h, c, n, C.byref(wp), s.cuda_stream), name)

                if args.once:
                    once(torch, launch, generic, affine)
                    continue
                us, reps = rate(torch, launch, args.seconds, first)
                first = False
                kernel = L.mi_blur_last_kernel().decode()
                gen_us, _ = rate(torch, generic, args.seconds, False)
                assert L.mi_blur_last_kernel().decode() == "blur_remap_generic_kernel"
                aff_us, _ = rate(torch, affine, args.seconds, False)
                assert L.mi_blur_last_kernel().decode() == "blur_warp_tiled_kernel"
                again, _ = rate(torch, launch, args.seconds, False)
                base = 0.5 * (us + again)
                spread = abs(us - again) / base
                moved, aff_moved = in_bytes + out_bytes + map_bytes, in_bytes + out_bytes
                tb, aff_tb = moved / (base * 1e-6) / 1e12, aff_moved / (aff_us * 1e-6) / 1e12
                print(f"{name:16s} {mname:7s} {stage or 65520:6d} | {us:9.1f} {again:9.1f} {tb:5.2f} {100 * spread:6.2f}% | {gen_us:10.1f} {gen_us / base:6.2f} | "
                      f"{aff_us:9.1f} {aff_tb:5.2f} {base / aff_us:12.2f} {moved / aff_moved:7.2f} | {plan['staged']:6d} {plan['direct']:6d} {plan['empty']:5d}  {kernel}", flush=True)
                rows.append({"point": name, "map": mname, "stage_bytes": stage or 65520, "launches": reps, "us": round(us, 2), "us_again": round(again, 2),
                             "spread": round(spread, 4), "tb_s": round(tb, 3), "generic_us": round(gen_us, 2), "generic_over_launch": round(gen_us / base, 3),
                             "affine_us": round(aff_us, 2), "affine_tb_s": round(aff_tb, 3), "launch_over_affine": round(base / aff_us, 3),
                             "traffic_over_affine": round(moved / aff_moved, 3), "plan": plan, "kernel": kernel})
            del d_map, d_map_off, flat
        del d_in, d_out
        torch.cuda.empty_cache()
    save(args, rows)


if __name__ == "__main__":
    main()
