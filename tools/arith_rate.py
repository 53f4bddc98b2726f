#!/usr/bin/env python3
"""Rate of the two-image arithmetic's kernels on one GPU (mi_blur_enqueue_arith), beside their own generic kernel on the
same buffers and beside two yardsticks in code this family does not touch, on the same A: the colour transform C -> C
with the identity matrix, and the plain 3x3 launch.

    python tools/arith_rate.py [--seconds 1.0] [--json FILE] [--once] [--lib PATH]

Per point five cases: ABSDIFF with a full B; LINEAR (the weights of add_weighted(0.7, 0.3)) with a full B; ABSDIFF against
a B shared by the batch; LERP through a plane mask (blur_arith_plane_kernel; blur_arith_flat_kernel for one channel,
where a plane is a full operand); LERP with every operand full.  Per point the two yardsticks are taken first, then per
case the launch, its generic kernel (the output pointer 1 byte off) and the launch again; each figure is calls back to
back on one stream for at least --seconds between two events (rate_common.py), us per call.  Only the first figure of a
point is preceded by a clock ramp of its own.  TB/s = the bytes of all operands plus the output / time (a shared operand
counted once per launch, as it is allocated); the yardsticks move 2 x the bytes of A.  The ratios compare TB/s: above 1
the case moves bytes faster than the yardstick.  The difference between the two figures of a launch is the spread any
gap has to exceed.
--once: five launches of each per point, in order, and nothing else (for a kernel trace or a counter run).
"""
import ctypes as C

from rate_common import once, rate, save, setup

# name, images, H, W, C
POINTS = [("1920x1080x3", 1, 1080, 1920, 3), ("4096x4096x1", 1, 4096, 4096, 1), ("4096x4096x4", 1, 4096, 4096, 4), ("256x256x3 x35", 35, 256, 256, 3)]


def main():
    args, torch, pkg, L = setup()
    rows = []
    print(f"{torch.cuda.get_device_name(0)}; >= {args.seconds:.1f} s of back-to-back calls per figure, after one ramp of the same length per point")
    print(f"{'point':14s} {'case':20s} | {'us':>8s} {'again':>8s} {'TB/s':>5s} {'spread':>7s} | {'generic us':>10s} {'x':>6s} | {'/colour':>7s} {'/3x3':>6s}  kernel")
    absdiff, lerp, weighted = pkg.arith_preset("absdiff"), pkg.arith_preset("lerp"), pkg.Arith()
    pkg.check(L.mi_blur_arith_weighted(0.7, 0.3, 0.0, C.byref(weighted)), "mi_blur_arith_weighted")
    shared = pkg.Arith.from_buffer_copy(absdiff)
    shared.b_shared = 1
    lerp_plane = pkg.Arith.from_buffer_copy(lerp)
    lerp_plane.m_plane = 1
    for name, n, h, w, c in POINTS:
        size, plane = n * h * w * c, n * h * w
        d_a, d_b, d_m = (torch.randint(0, 256, (size + 16,), dtype=torch.uint8, device="cuda") for _ in range(3))
        d_out = torch.empty((size + 16,), dtype=torch.uint8, device="cuda")
        ident = pkg.Color()
        pkg.check(L.mi_blur_color_identity(c, C.byref(ident)), "mi_blur_color_identity")
        s = torch.cuda.current_stream()
        pa, pb, pm, po = d_a.data_ptr(), d_b.data_ptr(), d_m.data_ptr(), d_out.data_ptr()

        def arith(k, mask, off):
            return lambda: pkg.check(L.mi_blur_enqueue_arith(pa, pb, mask, po + off, w, h, c, n, C.byref(k), s.cuda_stream), name)

        yard_colour = lambda: pkg.check(L.mi_blur_enqueue_color(pa, po, w, h, c, n, C.byref(ident), s.cuda_stream), name)
        yard_3x3 = lambda: pkg.check(L.mi_blur_enqueue(pa, po, w, h, c, 1, n, s.cuda_stream), name)
        # case, struct, mask, bytes of all operands plus the output
        cases = [("absdiff", absdiff, None, 3 * size), ("linear", weighted, None, 3 * size), ("absdiff shared B", shared, None, 2 * size + size // n),
                 ("lerp plane mask", lerp_plane, pm, 3 * size + plane), ("lerp", lerp, pm, 4 * size)]
        if args.once:
            once(torch, yard_colour, yard_3x3, *(f for _, k, mask, _ in cases for f in (arith(k, mask, 0), arith(k, mask, 1))))
            continue
        colour_us = rate(torch, yard_colour, args.seconds, True)[0]
        colour_kernel = L.mi_blur_last_kernel().decode()
        box_us = rate(torch, yard_3x3, args.seconds, False)[0]
        box_kernel = L.mi_blur_last_kernel().decode()
        colour_tb, box_tb = (2 * size / (us * 1e-6) / 1e12 for us in (colour_us, box_us))
        print(f"{name:14s} yardsticks: colour {colour_us:.1f} us {colour_tb:.2f} TB/s ({colour_kernel}), 3x3 {box_us:.1f} us {box_tb:.2f} TB/s ({box_kernel})", flush=True)
        for case, k, mask, moved in cases:
            us, reps = rate(torch, arith(k, mask, 0), args.seconds, False)
            kernel = L.mi_blur_last_kernel().decode()
            gen_us = rate(torch, arith(k, mask, 1), args.seconds, False)[0]
            assert L.mi_blur_last_kernel().decode() == "blur_arith_generic_kernel" and "generic" not in kernel
            again = rate(torch, arith(k, mask, 0), args.seconds, False)[0]
            base = 0.5 * (us + again)
            spread = abs(us - again) / base
            tb = moved / (base * 1e-6) / 1e12
            print(f"{name:14s} {case:20s} | {us:8.1f} {again:8.1f} {tb:5.2f} {100 * spread:6.2f}% | {gen_us:10.1f} {gen_us / base:6.2f} | "
                  f"{tb / colour_tb:7.3f} {tb / box_tb:6.3f}  {kernel}", flush=True)
            rows.append({"point": name, "case": case, "launches": reps, "us": round(us, 2), "us_again": round(again, 2), "spread": round(spread, 4),
                         "bytes": moved, "tb_s": round(tb, 3), "generic_us": round(gen_us, 2), "generic_over_launch": round(gen_us / base, 3), "kernel": kernel,
                         "colour_us": round(colour_us, 2), "colour_tb_s": round(colour_tb, 3), "rate_over_colour": round(tb / colour_tb, 3),
                         "box3x3_us": round(box_us, 2), "box3x3_tb_s": round(box_tb, 3), "rate_over_3x3": round(tb / box_tb, 3)})
        del d_a, d_b, d_m, d_out
        torch.cuda.empty_cache()
    save(args, rows)


if __name__ == "__main__":
    main()
