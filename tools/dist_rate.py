#!/usr/bin/env python3
"""Rate of the distance transform on one GPU (mi_blur_enqueue_dist, mi_blur_enqueue_dist_u8), beside its own generic row
pass on the same buffers and beside yardsticks in code this family does not touch, on the same input: the arithmetic flat
kernel (ABSDIFF), the plain 3x3 launch, the integral image S (the other reduce-then-scan family) and the 33 x 33 dilation
(mi_blur_enqueue_morph) against the chessboard disc of radius 16 (DIST_WITHIN).

    python tools/dist_rate.py [--seconds 1.0] [--json FILE] [--once] [--lib PATH]

Per point and per kind of data (random zeros at 20 % and at 1 %, one zero in a corner, none at all: the last two are the
worst cases of the pruned search): the L2 table and the L2 byte form, each timed twice; L1 and LINF tables; the byte form
through the generic row pass (the output 1 byte off); the table with the limits 16 and 255; on the 1 % data and the
corner the column pass's band ("dist_band") and the search chunk ("dist_chunk_log2") varied.  A worst-case launch is
first timed on its own: where one launch takes more than SLOW_MS (40 ms) the figure is that single launch (marked "single") and
the generic form is skipped; the points run from the smallest shape up, so the time of a larger one can be read off the
smaller ones before it starts.  Each other figure is calls back to back on one stream for at least --seconds between two
events (rate_common.py), us per call; only the first figure of a point is preceded by a clock ramp of its own.  The
bytes the design moves per element: the input twice, g written, read, written and read again (2 bytes each), the output
once (4 or 1): TB/s = that / time.  The three column-pass dispatches and the row pass are separate kernels: their split
is read from a kernel trace of --once (five launches of each form per point and kind, in order, and nothing else).
"""
import ctypes as C
import time

from rate_common import once, rate, save, setup

# name, images, H, W, C: from the smallest up
POINTS = [("256x256x3 x35", 35, 256, 256, 3), ("1920x1080x3", 1, 1080, 1920, 3), ("4096x4096x1", 1, 4096, 4096, 1), ("4096x4096x4", 1, 4096, 4096, 4)]
KINDS = ("random 20%", "random 1%", "corner", "none")
BANDS = (8, 16, 32, 64, 128)
CHUNKS = (3, 4, 5)
L2, L1, LINF = 0, 1, 2
BYTE, WITHIN = 0, 1
SLOW_MS = 40.0


def fill(torch, kind, size):
    d = torch.randint(1, 256, (size + 16,), dtype=torch.uint8, device="cuda")
    if kind.startswith("random"):
        share = 0.2 if "20" in kind else 0.01
        d[torch.rand((size + 16,), device="cuda") < share] = 0
    elif kind == "corner":
        d[0] = 0                                                           # channel 0 of image 0 alone has a site
    return d


def main():
    args, torch, pkg, L = setup()
    rows = []
    band0, chunk0 = 32, 4
    print(f"{torch.cuda.get_device_name(0)}; >= {args.seconds:.2f} s of back-to-back calls per figure, after one ramp of the same length per point")
    absdiff = pkg.arith_preset("absdiff")
    for name, n, h, w, c in POINTS:
        size = n * h * w * c
        d_b = torch.randint(0, 256, (size + 16,), dtype=torch.uint8, device="cuda")
        d_out = torch.empty((size + 16,), dtype=torch.uint8, device="cuda")
        d_t = torch.empty((size,), dtype=torch.int32, device="cuda")
        L.mi_blur_set_option(b"dist_band", 1)
        d_work = torch.empty((max(L.mi_blur_dist_work_bytes(w, h, c, n, C.byref(pkg.Dist(L2, 0, 0, 0, 0))), L.mi_blur_integral_work_bytes(w, h, c, n, 0)),),
                             dtype=torch.uint8, device="cuda")                # the largest any form here needs
        L.mi_blur_set_option(b"dist_band", band0)
        s = torch.cuda.current_stream()
        pb, po, pt, pw = d_b.data_ptr(), d_out.data_ptr(), d_t.data_ptr(), d_work.data_ptr()
        for kind in KINDS:
            d_in = fill(torch, kind, size)
            pi = d_in.data_ptr()

            def table(metric, limit=0):
                k = pkg.Dist(metric, 0, limit, 0, 0)
                return lambda: pkg.check(L.mi_blur_enqueue_dist(pi, pt, w, h, c, n, C.byref(k), pw, s.cuda_stream), name)

            def byte(metric, off=0, byte_op=BYTE, limit=0, nonzero=0):
                k = pkg.Dist(metric, nonzero, limit, byte_op, 0)
                return lambda: pkg.check(L.mi_blur_enqueue_dist_u8(pi, po + off, w, h, c, n, C.byref(k), pw, s.cuda_stream), name)

            yard_arith = lambda: pkg.check(L.mi_blur_enqueue_arith(pi, pb, None, po, w, h, c, n, C.byref(absdiff), s.cuda_stream), name)
            yard_3x3 = lambda: pkg.check(L.mi_blur_enqueue(pi, po, w, h, c, 1, n, s.cuda_stream), name)
            yard_integral = lambda: pkg.check(L.mi_blur_enqueue_integral(pi, pt, None, w, h, c, n, pw, s.cuda_stream), name)
            yard_dilate = lambda: pkg.check(L.mi_blur_enqueue_morph(pi, po, w, h, c, pkg.MORPH_DILATE, 16, 16, n, s.cuda_stream), name)
            disc = byte(LINF, 0, WITHIN, 16, 1)
            worst = kind in ("corner", "none")
            if args.once:
                once(torch, yard_arith, yard_3x3, yard_integral, yard_dilate, table(L2), byte(L2), table(L1), table(LINF), table(L2, 16), disc,
                     *(() if worst else (byte(L2, 1),)))
                continue

            def single(go):
                """One launch on its own, ms (after one that loads the code)."""
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                go()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            def t(go, ramp=False):
                """us per call; (us, True) from one launch where a launch is slow."""
                go()
                ms = single(go)
                if ms > SLOW_MS:
                    return ms * 1e3, True
                return rate(torch, go, args.seconds, ramp)[0], False

            row = {"point": name, "data": kind, "elements": size}
            if kind == KINDS[0]:
                yard = {}
                for label, go, moved in (("absdiff", yard_arith, 3 * size), ("3x3", yard_3x3, 2 * size), ("integral S", yard_integral, None), ("dilate 33x33", yard_dilate, 2 * size)):
                    us, _ = t(go, label == "absdiff")
                    yard[label] = {"us": round(us, 2), "kernel": L.mi_blur_last_kernel().decode(), "tb_s": round(moved / us / 1e6, 3) if moved else None}
                print(f"{name:14s} yardsticks: " + ", ".join(f"{k} {v['us']:.1f} us" + (f" {v['tb_s']:.2f} TB/s" if v['tb_s'] else "") + f" ({v['kernel']})" for k, v in yard.items()), flush=True)
                point_yard = yard
            row["yardsticks"] = point_yard
            forms = [("L2 table", table(L2), 4), ("L2 byte", byte(L2), 1), ("L1 table", table(L1), 4), ("LINF table", table(LINF), 4),
                     ("L2 table limit 16", table(L2, 16), 4), ("L2 table limit 255", table(L2, 255), 4), ("disc r16 linf", disc, 1)]
            res = {}
            for label, go, out_bytes in forms:
                us, slow = t(go)
                kernel = L.mi_blur_last_kernel().decode()
                again, _ = t(go) if label in ("L2 table", "L2 byte") else (us, slow)
                moved = size * (2 + 8 + out_bytes)
                base = 0.5 * (us + again)
                res[label] = {"us": round(us, 2), "us_again": round(again, 2), "single": slow, "bytes": moved, "tb_s": round(moved / base / 1e6, 4), "kernel": kernel}
                print(f"{name:14s} {kind:10s} {label:20s} | {us:10.1f} {again:10.1f} us{' single' if slow else ''}  {moved / base / 1e6:6.3f} TB/s  "
                      f"/ absdiff {moved / base / 1e6 / point_yard['absdiff']['tb_s']:5.3f}  / 3x3 {moved / base / 1e6 / point_yard['3x3']['tb_s']:5.3f}  "
                      f"time / integral S {base / point_yard['integral S']['us']:6.2f}  {kernel}", flush=True)
            row["forms"] = res
            row["disc_over_dilate33"] = round(res["disc r16 linf"]["us"] / point_yard["dilate 33x33"]["us"], 3)
            print(f"{name:14s} {kind:10s} disc r16 linf / dilate 33x33: {row['disc_over_dilate33']:.3f}", flush=True)
            if not res["L2 byte"]["single"] and not (worst and h * w > 256 * 256):
                us, slow = t(byte(L2, 1))
                assert L.mi_blur_last_kernel().decode() == "blur_dist_generic_kernel"
                row["generic_byte_us"], row["generic_single"] = round(us, 2), slow
                print(f"{name:14s} {kind:10s} L2 byte, generic row pass | {us:10.1f} us{' single' if slow else ''}  x{us / res['L2 byte']['us']:.2f}", flush=True)
            if kind in ("random 1%", "corner") and not res["L2 table"]["single"]:
                sweep = {}
                for band in BANDS:
                    L.mi_blur_set_option(b"dist_band", band)
                    sweep[band] = round(t(table(L2))[0], 2)
                L.mi_blur_set_option(b"dist_band", band0)
                row["band_us"] = sweep
                chunks = {}
                for log2 in CHUNKS:
                    L.mi_blur_set_option(b"dist_chunk_log2", log2)
                    chunks[1 << log2] = round(t(table(L2))[0], 2)
                L.mi_blur_set_option(b"dist_chunk_log2", chunk0)
                row["chunk_us"] = chunks
                print(f"{name:14s} {kind:10s} L2 table | rows per band -> us: {sweep} | columns per chunk -> us: {chunks}", flush=True)
            rows.append(row)
            save(args, rows)                                                   # what is measured so far survives a time limit
            del d_in
        del d_b, d_out, d_t, d_work
        torch.cuda.empty_cache()
    save(args, rows)


if __name__ == "__main__":
    main()
