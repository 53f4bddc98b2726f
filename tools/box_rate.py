#!/usr/bin/env python3
"""Rate of the integral image and of the box filters made from it on one GPU (mi_blur_enqueue_integral,
mi_blur_enqueue_box_from_integral, mi_blur_enqueue_box), beside their own generic kernels on the same buffers and beside
yardsticks in code this family does not touch, on the same input: the arithmetic flat kernel (ABSDIFF), the plain 3x3
launch, and (for the window of radius 16) the separable Gaussian of radius 16 (mi_blur_enqueue_sep).

    python tools/box_rate.py [--seconds 1.0] [--json FILE] [--once] [--lib PATH]

Per point: the two yardsticks; the integral for S alone and for S and Q together, each launch timed twice with its generic
form (the input pointer 1 byte off) between; the same two launches with bands of 8, 16, 32 and 64 rows ("integral_band");
the consumer alone from tables that are there, MEAN at r = 1, 16 and 127, with threads that own 16 bytes instead of 4 ("box_bytes") at r = 16 and 127,
STDDEV and THRESHOLD at r = 16, and its generic kernel (the output 1 byte off); the fused mi_blur_enqueue_box MEAN at
r = 1, 16 and 127, STDDEV and THRESHOLD at r = 16; the separable Gaussian of radius 16.  Each figure is calls back to
back on one stream for at least --seconds between two events (rate_common.py), us per call; only the first figure of a
point is preceded by a clock ramp of its own.  TB/s of the integral = (the input twice + the tables once + the work
buffer four times: written, prefixed in place, read) / time; the yardsticks move 2 x (3 x for ABSDIFF) the input's bytes.
The difference between the two figures of a launch is the spread any gap has to exceed.
--once: five launches of each form per point, in order, and nothing else (for a kernel trace or a counter run).
"""
import ctypes as C

from rate_common import once, rate, save, setup

# name, images, H, W, C
POINTS = [("1920x1080x3", 1, 1080, 1920, 3), ("4096x4096x1", 1, 4096, 4096, 1), ("4096x4096x4", 1, 4096, 4096, 4), ("256x256x3 x35", 35, 256, 256, 3)]
BANDS = (8, 16, 32, 64)
MEAN, STDDEV, THRESHOLD = 0, 1, 2


def main():
    args, torch, pkg, L = setup()
    rows = []
    band0 = 16
    print(f"{torch.cuda.get_device_name(0)}; >= {args.seconds:.2f} s of back-to-back calls per figure, after one ramp of the same length per point")
    absdiff = pkg.arith_preset("absdiff")
    gauss = pkg.SepKernel()
    pkg.check(L.mi_blur_sep_kernel_gauss(8.0, 0.0, 16, 8, C.byref(gauss)), "mi_blur_sep_kernel_gauss")
    for name, n, h, w, c in POINTS:
        size = n * h * w * c
        d_in, d_b = (torch.randint(0, 256, (size + 16,), dtype=torch.uint8, device="cuda") for _ in range(2))
        d_out = torch.empty((size + 16,), dtype=torch.uint8, device="cuda")
        d_s, d_q = (torch.empty((size,), dtype=torch.int32, device="cuda") for _ in range(2))
        L.mi_blur_set_option(b"integral_band", min(BANDS))
        big = pkg.Box(STDDEV, 1, 1, 0, 0)
        d_work = torch.empty((L.mi_blur_box_work_bytes(w, h, c, n, C.byref(big)),), dtype=torch.uint8, device="cuda")     # the largest any form here needs
        L.mi_blur_set_option(b"integral_band", band0)
        s = torch.cuda.current_stream()
        pi, pb, po, ps, pq, pw = d_in.data_ptr(), d_b.data_ptr(), d_out.data_ptr(), d_s.data_ptr(), d_q.data_ptr(), d_work.data_ptr()

        def integral(both, off=0):
            return lambda: pkg.check(L.mi_blur_enqueue_integral(pi + off, ps, pq if both else None, w, h, c, n, pw, s.cuda_stream), name)

        def consumer(k, off=0):
            return lambda: pkg.check(L.mi_blur_enqueue_box_from_integral(pi if k.op == THRESHOLD else None, ps, pq if k.op == STDDEV else None, po + off,
                                                                         w, h, c, n, C.byref(k), s.cuda_stream), name)

        def fused(k):
            return lambda: pkg.check(L.mi_blur_enqueue_box(pi, po, w, h, c, n, C.byref(k), pw, s.cuda_stream), name)

        yard_arith = lambda: pkg.check(L.mi_blur_enqueue_arith(pi, pb, None, po, w, h, c, n, C.byref(absdiff), s.cuda_stream), name)
        yard_3x3 = lambda: pkg.check(L.mi_blur_enqueue(pi, po, w, h, c, 1, n, s.cuda_stream), name)
        yard_sep = lambda: pkg.check(L.mi_blur_enqueue_sep(pi, po, w, h, c, n, C.byref(gauss), s.cuda_stream), name)
        box = lambda op, r: pkg.Box(op, r, r, 5 if op == THRESHOLD else 0, 0)
        if args.once:
            once(torch, yard_arith, yard_3x3, yard_sep, integral(False), integral(True), integral(False, 1), integral(True, 1),
                 *(consumer(box(MEAN, r)) for r in (1, 16, 127)), consumer(box(STDDEV, 16)), consumer(box(THRESHOLD, 16)), consumer(box(MEAN, 16), 1),
                 *(fused(box(MEAN, r)) for r in (1, 16, 127)))
            continue
        t = lambda go, ramp=False: rate(torch, go, args.seconds, ramp)[0]
        row = {"point": name, "bytes": size}
        row["arith_us"] = t(yard_arith, True)
        row["arith_kernel"] = L.mi_blur_last_kernel().decode()
        row["box3x3_us"] = t(yard_3x3)
        row["box3x3_kernel"] = L.mi_blur_last_kernel().decode()
        row["sep16_us"], row["sep16_radius"] = t(yard_sep), gauss.rx
        arith_tb, box_tb = 3 * size / row["arith_us"] / 1e6, 2 * size / row["box3x3_us"] / 1e6
        print(f"{name:14s} yardsticks: absdiff {row['arith_us']:.1f} us {arith_tb:.2f} TB/s ({row['arith_kernel']}), 3x3 {row['box3x3_us']:.1f} us {box_tb:.2f} TB/s "
              f"({row['box3x3_kernel']}), gaussian r{gauss.rx} {row['sep16_us']:.1f} us", flush=True)
        for both in (False, True):
            tag = "S+Q" if both else "S"
            us = t(integral(both))
            kernel = L.mi_blur_last_kernel().decode()
            gen = t(integral(both, 1))
            assert L.mi_blur_last_kernel().decode() == "blur_integral_generic_kernel" and "generic" not in kernel
            again = t(integral(both))
            base = 0.5 * (us + again)
            moved = 2 * size + (2 if both else 1) * 4 * size + 4 * L.mi_blur_integral_work_bytes(w, h, c, n, int(both))
            tb = moved / base / 1e6
            print(f"{name:14s} integral {tag:4s} | {us:8.1f} {again:8.1f} us  {tb:5.2f} TB/s  spread {100 * abs(us - again) / base:5.2f}% | generic {gen:9.1f} us "
                  f"x{gen / base:6.2f} | rate / absdiff {tb / arith_tb:5.3f}  / 3x3 {tb / box_tb:5.3f}  {kernel}", flush=True)
            row[f"integral_{tag}"] = {"us": round(us, 2), "us_again": round(again, 2), "bytes": moved, "tb_s": round(tb, 3), "generic_us": round(gen, 2),
                                      "rate_over_absdiff": round(tb / arith_tb, 3), "rate_over_3x3": round(tb / box_tb, 3), "kernel": kernel}
            sweep = {}
            for band in BANDS:
                L.mi_blur_set_option(b"integral_band", band)
                sweep[band] = round(t(integral(both)), 2)
            L.mi_blur_set_option(b"integral_band", band0)
            print(f"{name:14s} integral {tag:4s} | rows per band -> us: {sweep}", flush=True)
            row[f"integral_{tag}"]["band_us"] = sweep
        integral(True)()                                                   # the tables the consumer reads
        cons = {}
        for label, k, fetch, off in [("mean r1", box(MEAN, 1), 4, 0), ("mean r16", box(MEAN, 16), 4, 0), ("mean r127", box(MEAN, 127), 4, 0),
                                     ("mean r16 16 B/thread", box(MEAN, 16), 16, 0), ("mean r127 16 B/thread", box(MEAN, 127), 16, 0),
                                     ("stddev r16", box(STDDEV, 16), 4, 0), ("stddev r16 16 B/thread", box(STDDEV, 16), 16, 0),
                                     ("threshold r16", box(THRESHOLD, 16), 4, 0), ("mean r16 generic", box(MEAN, 16), 4, 1)]:
            L.mi_blur_set_option(b"box_bytes", fetch)
            us = t(consumer(k, off))
            kernel = L.mi_blur_last_kernel().decode()
            again = t(consumer(k, off))
            cons[label] = {"us": round(us, 2), "us_again": round(again, 2), "kernel": kernel}
            print(f"{name:14s} consumer {label:24s} | {us:8.1f} {again:8.1f} us  {kernel}", flush=True)
        L.mi_blur_set_option(b"box_bytes", 4)
        row["consumer"] = cons
        fus = {}
        for label, k in [("mean r1", box(MEAN, 1)), ("mean r16", box(MEAN, 16)), ("mean r127", box(MEAN, 127)), ("stddev r16", box(STDDEV, 16)),
                         ("threshold r16", box(THRESHOLD, 16))]:
            us = t(fused(k))
            again = t(fused(k))
            fus[label] = {"us": round(us, 2), "us_again": round(again, 2)}
            print(f"{name:14s} fused    {label:24s} | {us:8.1f} {again:8.1f} us", flush=True)
        row["fused"] = fus
        m = lambda d, key: 0.5 * (d[key]["us"] + d[key]["us_again"])
        row["consumer_r127_over_r1"] = round(m(cons, "mean r127") / m(cons, "mean r1"), 3)
        row["fused_r127_over_r1"] = round(m(fus, "mean r127") / m(fus, "mean r1"), 3)
        row["fused_r16_over_sep16"] = round(m(fus, "mean r16") / row["sep16_us"], 3)
        print(f"{name:14s} time(r = 127) / time(r = 1): consumer {row['consumer_r127_over_r1']:.3f}, fused {row['fused_r127_over_r1']:.3f}; "
              f"fused mean r16 / gaussian r{gauss.rx}: {row['fused_r16_over_sep16']:.3f}", flush=True)
        rows.append(row)
        del d_in, d_b, d_out, d_s, d_q, d_work
        torch.cuda.empty_cache()
    save(args, rows)


if __name__ == "__main__":
    main()
