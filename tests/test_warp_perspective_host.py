"""The perspective warp (mi_blur_warp_perspective_coord, _quad, _set_matrix, mi_blur_cpu_run_warp_perspective,
mi_blur_enqueue_warp_perspective's argument checks, mi_blur_ctx_set_warp_perspective, warp_perspective() /
perspective_matrix() / warp_perspective_coord(), the hosts' --perspective), CPU only: against the numpy restatement of the
header's definition (warp_perspective_ref.py), independent of the product.  All comparisons are exact unless stated."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from filter_harness import MEDIAN, cpu_run as cpu_run_same_size
from resample_harness import (PERSP, WARP, check_cpu_context, check_cpu_run_refuses, check_ctx_set_refuses, check_enqueue_invalid_before_no_device,
                              check_setters_replace_each_other, cpu_run, needs_gxx, run_sanitized, sampler_rows, size_rows)
from warp_ref import LIMIT_FILL, LIMIT_MAPS as AFFINE_LIMIT_MAPS, TILED_SHAPES, limit_image, limit_out, make_warp, ref_warp as ref_affine, rotation_m, quantise
from warp_perspective_ref import (BIG_QUAD, BILINEAR, CLAMP, CONSTANT, EXTREME, LIMIT_MAPS, LIN_MAX, MAX_DIM, NAMED, NEAREST, OFF_MAX, Q, affine_h,
                                  box, float_warp, fraction_bits, limit_references, make_persp, max_footprint, named_maps, named_quads,
                                  normalised, out_corners, outside_share, quad_forward, quad_h, ref_coord, ref_warp, set_matrix, takes_tiled,
                                  tile_footprints, tiles, valid)

MODES = (BILINEAR, NEAREST)
BORDERS = (CLAMP, CONSTANT)


def coord(L, wp, X, Y):
    x0, y0, fx, fy = C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
    rc = L.mi_blur_warp_perspective_coord(C.byref(wp), X, Y, C.byref(x0), C.byref(y0), C.byref(fx), C.byref(fy))
    return rc, (x0.value, y0.value, fx.value, fy.value)


def set_h(pkg, L, H, inverse, wo, ho):
    """(status, h) of mi_blur_warp_perspective_set_matrix on a struct whose h starts as nine 7s."""
    wp = make_persp(pkg, [7] * 9, wo, ho)
    rc = L.mi_blur_warp_perspective_set_matrix(C.byref(wp), (C.c_double * 9)(*[float(v) for v in H]), int(inverse))
    return rc, list(wp.h)


def random_quad_h(rng, w, h, wo, ho):
    """A valid homography from a random convex-ish source quad around the image, or None."""
    base = np.array([(0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1)], dtype=np.float64)
    quad = base + rng.uniform(-0.45, 0.45, size=(4, 2)) * np.array([w, h])
    try:
        got = set_matrix(quad_forward([tuple(p) for p in quad], out_corners(wo, ho)), False, wo, ho)
    except np.linalg.LinAlgError:
        return None
    return None if got is None else got[0]


def test_the_named_maps_are_what_the_gpu_tests_need():
    """On the restatement alone: valid at 30 fraction bits, tiled under both borders within 7040 bytes, the outside shares,
    and footprints that differ from tile to tile where the map is strongly projective."""
    for shape, (wo, ho) in TILED_SHAPES:
        n, h, w, c = shape
        for name, quad in named_quads(w, h).items():
            hh, k = set_matrix(quad_forward(quad, out_corners(wo, ho)), False, wo, ho)
            assert k == 30 and valid(hh, wo, ho), name
        maps = named_maps(w, h, wo, ho)
        for name in NAMED:
            hh = maps[name]
            share = outside_share(hh, BILINEAR, w, h, wo, ho)
            assert share == 1.0 if name == "outside" else share < 0.5, (name, share)
            assert name == "affine" or (share > 0.1) == (name in ("half-out", "outside")), (name, share)   # the rotation leaves the output's corners empty
            for border in BORDERS:
                assert takes_tiled(shape, hh, wo, ho, BILINEAR, border), (name, border)
                assert name == "affine" or max_footprint(shape, hh, wo, ho, border) <= 7040, (name, border)      # the quads; the rotation stages up to 9024 bytes
            if name in ("keystone", "steep"):
                assert len({f for f in tile_footprints(shape, hh, wo, ho, CONSTANT) if f}) > 1, name
    big = (1, 512, 512, 1)
    assert max_footprint(big, quad_h(512, 512, 64, 64, BIG_QUAD), 64, 64, CLAMP) == 161280
    assert max_footprint(big, quad_h(512, 512, 128, 128, BIG_QUAD), 128, 128, CLAMP) == 45824
    for ishape, (wo, ho), hh, border in EXTREME:
        for b in BORDERS if border is None else (border,):
            assert valid(hh, wo, ho) and takes_tiled((1,) + ishape, hh, wo, ho, BILINEAR, b)


def test_coord_equals_the_restatement(pkg, L):
    rng = np.random.default_rng(1)
    maps = [affine_h([Q, 0, 0, 0, Q, 0]), [LIN_MAX, -LIN_MAX, OFF_MAX, -LIN_MAX, LIN_MAX, -OFF_MAX, LIN_MAX, LIN_MAX, OFF_MAX],
            [-LIN_MAX, -LIN_MAX, -OFF_MAX, LIN_MAX, LIN_MAX, OFF_MAX, 0, 0, 1], [0] * 8 + [1], [5, -3, 2, 7, 1, -9, 0, 0, 4]]
    maps += [hf(96) for hf, _, _, _ in LIMIT_MAPS.values()]
    maps += list(named_maps(96, 80, 144, 70).values())
    for _ in range(30):
        lin = rng.integers(-LIN_MAX, LIN_MAX + 1, size=4)
        off = rng.integers(-OFF_MAX, OFF_MAX + 1, size=2)
        den = rng.integers(0, LIN_MAX + 1, size=2)
        maps.append([int(lin[0]), int(lin[1]), int(off[0]), int(lin[2]), int(lin[3]), int(off[1]), int(den[0]), int(den[1]), int(rng.integers(1, OFF_MAX + 1))])
    grid = [(X, Y) for X in (0, 1, 13, 79, 95) for Y in (0, 1, 7, 39)] + [(MAX_DIM - 1, MAX_DIM - 1), (MAX_DIM - 1, 0), (0, MAX_DIM - 1)]
    checked = 0
    for h in maps:
        for mode in MODES:
            wp = make_persp(pkg, h, 1, 1, mode)
            for X, Y in grid:
                d = h[6] * X + h[7] * Y + h[8]
                rc, got = coord(L, wp, X, Y)
                if d < 1:
                    assert rc == pkg.ERR_INVALID, (h, X, Y)
                    continue
                want = tuple(int(v) for v in ref_coord(h, mode, X, Y))
                assert rc == pkg.OK and got == want, (h, mode, X, Y)
                assert 0 <= got[2] <= 2047 and 0 <= got[3] <= 2047 and (mode == BILINEAR or got[2:] == (0, 0))
                assert pkg.warp_perspective_coord(wp, X, Y) == want
                checked += 1
    assert checked > 1000
    good = make_persp(pkg, affine_h([Q, 0, 0, 0, Q, 0]), 1, 1)
    for X, Y in ((-1, 0), (0, -1), (MAX_DIM, 0), (0, MAX_DIM)):
        assert coord(L, good, X, Y)[0] == pkg.ERR_INVALID
    x0, y0, fx, fy = C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
    assert L.mi_blur_warp_perspective_coord(None, 0, 0, C.byref(x0), C.byref(y0), C.byref(fx), C.byref(fy)) == pkg.ERR_INVALID
    assert L.mi_blur_warp_perspective_coord(C.byref(good), 0, 0, None, C.byref(y0), C.byref(fx), C.byref(fy)) == pkg.ERR_INVALID
    assert coord(L, make_persp(pkg, affine_h([Q, 0, 0, 0, Q, 0]), 1, 1, 2), 0, 0)[0] == pkg.ERR_INVALID
    for i, lim in ((1, LIN_MAX), (7, LIN_MAX), (5, OFF_MAX), (8, OFF_MAX)):
        over = [Q, 0, 0, 0, Q, 0, 0, 0, Q]
        over[i] = lim + 1
        assert coord(L, make_persp(pkg, over, 1, 1), 0, 0)[0] == pkg.ERR_INVALID, i
        over[i] = lim
        assert coord(L, make_persp(pkg, over, 1, 1), 0, 0)[0] == pkg.OK, i
    assert coord(L, make_persp(pkg, [Q, 0, 0, 0, Q, 0, 0, 0, 0], 1, 1), 0, 0)[0] == pkg.ERR_INVALID       # h8 = 0


def test_set_matrix_exact_entries(pkg, L):
    # inverse != 0: the entries are v * 2^k, exactly representable here
    for H, wo, ho in (([1, 0, 0, 0, 1, 0, 0, 0, 1], 64, 48), ([0.5, 0.25, -3.0, -0.125, 2.0, 7.5, 2.0 ** -10, -2.0 ** -11, 1.0], 64, 48),
                      ([2, 0, 10, 0, 2, -6, 0, 0, 2], 640, 480), ([3.0, 1.0, 100.0, -2.0, 5.0, 17.0, 2.0 ** -12, 0.0, 4.0], 100, 100)):
        rc, h = set_h(pkg, L, H, 1, wo, ho)
        v = [x / H[8] for x in H]
        k = fraction_bits(v)
        assert rc == pkg.OK and h == [int(x * 2 ** k) for x in v] and all(x * 2 ** k == int(x * 2 ** k) for x in v), H
        assert set_matrix(H, True, wo, ho) == (h, k)
    assert set_h(pkg, L, [1, 0, 0, 0, 1, 0, 0, 0, 1], 1, 8, 8)[1] == [1 << 30, 0, 0, 0, 1 << 30, 0, 0, 0, 1 << 30]
    # inverse == 0 with an exactly representable inverse and normalisation: power-of-two scales, integer shifts, perspective terms 2^-10
    for fwd, want_v in (([2, 0, 0, 0, 4, 0, 0, 0, 1], [0.5, 0, 0, 0, 0.25, 0, 0, 0, 1]),
                        ([1, 0, 5, 0, 1, -3, 0, 0, 1], [1, 0, -5, 0, 1, 3, 0, 0, 1]),
                        ([0.5, 0, 8, 0, 0.5, 16, 0, 0, 1], [2, 0, -16, 0, 2, -32, 0, 0, 1]),
                        ([1, 0, 0, 0, 1, 0, 2.0 ** -10, 0, 1], [1, 0, 0, 0, 1, 0, -2.0 ** -10, 0, 1])):
        rc, h = set_h(pkg, L, fwd, 0, 64, 48)
        k = fraction_bits(want_v)
        assert rc == pkg.OK and h == [int(x * 2 ** k) for x in want_v], fwd
        assert normalised(fwd, False) == [float(x) for x in want_v] and set_matrix(fwd, False, 64, 48) == (h, k)
    # k as specified: a shift of 2^20 leaves 2^48 / 2^20 = 28 bits less one
    rc, h = set_h(pkg, L, [1, 0, 2.0 ** 20, 0, 1, 0, 0, 0, 1], 1, 8, 8)
    assert rc == pkg.OK and h == [1 << 27, 0, 1 << 47, 0, 1 << 27, 0, 0, 0, 1 << 27] and fraction_bits([1, 0, 2.0 ** 20, 0, 1, 0, 0, 0, 1]) == 27
    rc, h = set_h(pkg, L, [8, 0, 0, 0, 1, 0, 0, 0, 1], 1, 8, 8)                          # 8 * 2^29 = 2^32 is over limit - 1
    assert rc == pkg.OK and h[0] == 8 << 28 and h[8] == 1 << 28
    rc, h = set_h(pkg, L, [2.0 ** 32 - 1, 0, 0, 0, 1, 0, 0, 0, 1], 1, 8, 8)                # k = 0
    assert rc == pkg.OK and h == [(1 << 32) - 1, 0, 0, 0, 1, 0, 0, 0, 1]


def test_set_matrix_general_quads(pkg, L):
    """The library's entries equal the restated setter's, and the four output corners land within 2^-16 pixel (one Q16
    quantum of the affine matrix) of where the float64 matrix puts them.

    What the number format gives: every entry is off by at most 2^-(k+1) of h8, so at output pixel (X, Y) the numerator
    and the denominator are each off by at most e = (X + Y + 1) * 2^-(k+1), and the position N / D by at most
    e * (1 + |N / D|) / (D / h8), D taken as low as the error can make it.  The 2^-16 bound follows from that only while
    (X + Y + 1) * (1 + |position|) / (D / h8) <= 2^(k - 15): small images, or mild perspective.  So every quad is held to
    the format's bound, the quads inside that domain (at least 40 of them, sizes up to 64) to 2^-16, and the domain is
    decided from the float64 matrix alone.  The named maps on 96 x 80 lie outside it: `steep` is off by 2.1e-5 pixel at
    its bottom-right corner (D / h8 = 0.1 there), which is the format's doing (the restated setter gives the same entries)."""
    rng = np.random.default_rng(5)
    cases = [(96, 80, wo, ho, quad) for (_, (wo, ho)) in TILED_SHAPES for quad in named_quads(96, 80).values()]
    for i in range(120):
        w, h, wo, ho = (int(v) for v in rng.integers(8, 2000 if i < 30 else 64, size=4))
        base = np.array([(0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1)], dtype=np.float64)
        cases.append((w, h, wo, ho, [tuple(p) for p in base + rng.uniform(-0.3, 0.3, size=(4, 2)) * np.array([w, h])]))
    seen = inside = 0
    for w, h, wo, ho, quad in cases:
        fwd = quad_forward(quad, out_corners(wo, ho))
        want = set_matrix(fwd, False, wo, ho)
        rc, got = set_h(pkg, L, fwd, 0, wo, ho)
        if want is None:
            assert rc == pkg.ERR_INVALID and got == [7] * 9
            continue
        assert rc == pkg.OK and got == want[0], quad
        v, k = normalised(fwd, False), want[1]
        in_domain, errs = True, []
        for (X, Y), (sx, sy) in zip(out_corners(wo, ho), quad):
            d = v[6] * X + v[7] * Y + v[8]
            fx, fy = (v[0] * X + v[1] * Y + v[2]) / d, (v[3] * X + v[4] * Y + v[5]) / d
            assert abs(fx - sx) <= 1e-6 and abs(fy - sy) <= 1e-6
            qd = got[6] * int(X) + got[7] * int(Y) + got[8]
            qx, qy = (got[0] * int(X) + got[1] * int(Y) + got[2]) / qd, (got[3] * int(X) + got[4] * int(Y) + got[5]) / qd
            e = (X + Y + 1) * 2.0 ** -(k + 1)
            for f, q in ((fx, qx), (fy, qy)):
                assert abs(q - f) <= e * (1 + abs(f)) / (d - e) + 1e-9, (quad, X, Y)
                in_domain = in_domain and (X + Y + 1) * (1 + abs(f)) / d <= 2.0 ** (k - 15) * 0.99
                errs.append(abs(q - f))
        if in_domain:
            assert max(errs) <= 2.0 ** -16, (quad, max(errs))
            inside += 1
        seen += 1
    assert seen >= 100 and inside >= 40, (seen, inside)


def test_set_matrix_refuses(pkg, L):
    inf, nan = float("inf"), float("nan")
    ident = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    bad = [([1, 2, 3, 2, 4, 6, 0, 0, 1], 0), ([0] * 9, 0), ([1, 0, 0, 0, 1, 0, 0, 0, 0], 1),       # singular; H[8] = 0
           ([1, 0, 5, 0, 1, 5, 1, 1, 0], 1),
           ([nan] + ident[1:], 1), (ident[:4] + [inf] + ident[5:], 0), ([1e200, 0, 0, 0, 1e200, 0, 0, 0, 1e200], 0),   # the determinant is not finite
           ([2.0 ** 32, 0, 0, 0, 1, 0, 0, 0, 1], 1), ([1, 0, 2.0 ** 48, 0, 1, 0, 0, 0, 1], 1), ([1, 0, 0, 0, 1, 0, 2.0 ** 32, 0, 1], 1),   # over a limit at k = 0
           ([1, 0, 0, 0, 1, 0, -1.0 / 32, 0, 1], 1),                                              # the horizon at X = 32, inside a 64-wide output
           ([1, 0, 0, 0, 1, 0, 0, -1.0 / 47, 1], 1)]                                              # D = 0 in the last row of 48
    for H, inverse in bad:
        rc, h = set_h(pkg, L, H, inverse, 64, 48)
        assert rc == pkg.ERR_INVALID and h == [7] * 9, H
        assert set_matrix(H, bool(inverse), 64, 48) is None, H
    assert set_h(pkg, L, [1, 0, 0, 0, 1, 0, -1.0 / 32, 0, 1], 1, 32, 48)[0] == pkg.OK              # the same map on an output that ends before it
    assert set_h(pkg, L, ident, 1, 0, 48)[0] == pkg.ERR_INVALID and set_h(pkg, L, ident, 1, 64, MAX_DIM + 1)[0] == pkg.ERR_INVALID
    wp = make_persp(pkg, [7] * 9, 64, 48)
    assert L.mi_blur_warp_perspective_set_matrix(None, (C.c_double * 9)(*ident), 1) == pkg.ERR_INVALID
    assert L.mi_blur_warp_perspective_set_matrix(C.byref(wp), None, 1) == pkg.ERR_INVALID


def test_quad_against_numpy_solve(pkg, L):
    rng = np.random.default_rng(7)
    H = (C.c_double * 9)()
    for _ in range(50):
        src = rng.uniform(-50, 1000, size=(4, 2)) if rng.random() < 0.3 else np.array([(0, 0), (639, 0), (639, 479), (0, 479)]) + rng.uniform(-150, 150, size=(4, 2))
        dst = np.array([(0, 0), (799, 0), (799, 599), (0, 599)], dtype=np.float64) + rng.uniform(-100, 100, size=(4, 2))
        try:
            want = quad_forward([tuple(p) for p in src], [tuple(p) for p in dst])
        except np.linalg.LinAlgError:
            continue
        rc = L.mi_blur_warp_perspective_quad((C.c_double * 8)(*src.reshape(-1)), (C.c_double * 8)(*dst.reshape(-1)), H)
        if rc != pkg.OK:
            assert np.linalg.cond(np.array(want).reshape(3, 3)) > 1e9
            continue
        got = list(H)
        assert got[8] == 1.0
        for (x, y), (u, v) in zip(src, dst):
            for M in (got, want):
                d = M[6] * x + M[7] * y + M[8]
                assert abs((M[0] * x + M[1] * y + M[2]) / d - u) <= 1e-6 and abs((M[3] * x + M[4] * y + M[5]) / d - v) <= 1e-6
        assert pkg.perspective_matrix(src, dst) == [got[0:3], got[3:6], got[6:9]]
    sq = [0, 0, 10, 0, 10, 10, 0, 10]
    assert L.mi_blur_warp_perspective_quad((C.c_double * 8)(*sq), (C.c_double * 8)(*sq), H) == pkg.OK
    assert np.allclose(list(H), [1, 0, 0, 0, 1, 0, 0, 0, 1], atol=1e-12)
    for bad in ([0, 0, 5, 0, 10, 0, 0, 10], [0, 0, 10, 0, 10, 10, 5, 5], [0, 0, 0, 0, 10, 10, 0, 10], [0, 0, float("nan"), 0, 10, 10, 0, 10],
                [0, 0, float("inf"), 0, 10, 10, 0, 10]):                      # three in line (twice), a repeated point, non-finite values
        assert L.mi_blur_warp_perspective_quad((C.c_double * 8)(*bad), (C.c_double * 8)(*sq), H) == pkg.ERR_INVALID, bad
        assert L.mi_blur_warp_perspective_quad((C.c_double * 8)(*sq), (C.c_double * 8)(*bad), H) == pkg.ERR_INVALID, bad
    assert L.mi_blur_warp_perspective_quad(None, (C.c_double * 8)(*sq), H) == pkg.ERR_INVALID
    assert L.mi_blur_warp_perspective_quad((C.c_double * 8)(*sq), (C.c_double * 8)(*sq), None) == pkg.ERR_INVALID
    with pytest.raises(ValueError):
        pkg.perspective_matrix([(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 0), (1, 1), (0, 1)])


@pytest.mark.parametrize("case", TILED_SHAPES, ids=lambda c: "x".join(map(str, c[0])) + f"-{c[1][0]}x{c[1][1]}")
def test_cpu_device_named_maps(pkg, L, case):
    shape, (wo, ho) = case
    n, h, w, c = shape
    img = np.random.default_rng(sum(shape)).integers(0, 256, size=shape, dtype=np.uint8)
    img[0, 0], img[0, -1], img[0, :, 0], img[0, :, -1] = 255, 0, 0, 255
    for name, hh in named_maps(w, h, wo, ho).items():
        for mode in MODES:
            for border in BORDERS:
                got = cpu_run(PERSP, pkg, L, img, (hh, wo, ho, mode, border, 173), 3)
                assert np.array_equal(got, ref_warp(img, hh, wo, ho, mode, border, 173)), (name, mode, border)


@pytest.mark.parametrize("c", [1, 2, 3, 4, 5])
def test_cpu_device_limit_maps(pkg, L, c):
    img, refs = limit_references(2, c)
    wo, ho = limit_out(c)
    for name, (hf, _, _, _) in LIMIT_MAPS.items():
        for mode in MODES:
            for border in BORDERS:
                for nt in (1, 5):
                    got = cpu_run(PERSP, pkg, L, img, (hf(wo), wo, ho, mode, border, LIMIT_FILL), nt)
                    assert np.array_equal(got, refs[name, mode, border]), (name, mode, border, nt)


def test_cpu_device_odd_shapes_and_thread_counts(pkg, L):
    rng = np.random.default_rng(3)
    for (n, h, w, c), (wo, ho) in (((2, 17, 33, 3), (48, 29)), ((1, 1, 1, 3), (9, 9)), ((2, 9, 5, 1), (11, 17)), ((1, 40, 50, 2), (1, 1)),
                                   ((1, 24, 64, 5), (37, 48)), ((3, 1, 7, 4), (5, 1)), ((1, 7, 1, 2), (1, 13))):
        img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
        maps = [affine_h(rotation_m(w, h, 30.0)), [3, 0, -7, 0, 2, 5, 0, 0, 1], [Q, 0, 0, 0, Q, 0, Q // 64, Q // 128, Q]]
        if wo > 1 and ho > 1:
            maps += [named_maps(max(w, 2), max(h, 2), wo, ho)[k] for k in ("keystone", "half-out")]
        for hh in maps:
            assert valid(hh, wo, ho)
            for mode in MODES:
                for border in BORDERS:
                    want = ref_warp(img, hh, wo, ho, mode, border, 99)
                    for nt in (1, 2, 7):
                        assert np.array_equal(cpu_run(PERSP, pkg, L, img, (hh, wo, ho, mode, border, 99), nt), want), ((n, h, w, c), hh, mode, border, nt)
    for ishape, (wo, ho), hh, border in EXTREME:                                 # the extreme shapes of the GPU tests
        img = rng.integers(0, 256, size=(1,) + ishape, dtype=np.uint8)
        for b in BORDERS if border is None else (border,):
            assert np.array_equal(cpu_run(PERSP, pkg, L, img, (hh, wo, ho, BILINEAR, b, 7), 4), ref_warp(img, hh, wo, ho, BILINEAR, b, 7))
    assert L.mi_blur_cpu_run_warp_perspective(img.ctypes.data, img.ctypes.data, 16, 32768, 1, 1, C.byref(make_persp(pkg, EXTREME[1][2], 16, 32768)), 1) == pkg.ERR_INVALID   # in == out


def test_affine_homographies_give_the_affine_warp(pkg, L):
    """h = {s m, 0, 0, s Q} is mi_blur_cpu_run_warp with m, for s = 1, 3, 2^14 and for the affine limit maps (s = 1: their
    entries times 2^14 would pass 2^32)."""
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, size=(2, 37, 42, 3), dtype=np.uint8)
    mats = [rotation_m(42, 37, 25.0, 1.1), quantise([0.8, 0.3, -20.5, -0.2, 0.7, 31.25]), [Q, 0, 3 * Q // 8 + 1, 0, Q, -5 * Q // 8 - 1], [0, 0, 10 * Q + 777, 0, 0, 20 * Q + 31111]]
    for m in mats:
        for s in (1, 3, 1 << 14):
            hh = affine_h(m, s)
            assert valid(hh, 63, 50), (m, s)
            for mode in MODES:
                for border in BORDERS:
                    want = cpu_run(WARP, pkg, L, img, (m, 63, 50, mode, border, 33), 2)
                    assert np.array_equal(want, ref_affine(img, m, 63, 50, mode, border, 33))
                    assert np.array_equal(ref_warp(img, hh, 63, 50, mode, border, 33), want), (m, s, mode, border)
                    assert np.array_equal(cpu_run(PERSP, pkg, L, img, (hh, 63, 50, mode, border, 33), 2), want), (m, s, mode, border)
    lim = limit_image(2, 3)
    wo, ho = limit_out(3)
    for name, (m, _, _) in AFFINE_LIMIT_MAPS.items():
        hh = affine_h(m)
        assert valid(hh, wo, ho), name
        for mode in MODES:
            for border in BORDERS:
                want = cpu_run(WARP, pkg, L, lim, (m, wo, ho, mode, border, LIMIT_FILL), 2)
                assert np.array_equal(ref_warp(lim, hh, wo, ho, mode, border, LIMIT_FILL), want), (name, mode, border)
                assert np.array_equal(cpu_run(PERSP, pkg, L, lim, (hh, wo, ho, mode, border, LIMIT_FILL), 2), want), (name, mode, border)


def test_a_rectangles_taps_lie_in_the_box_of_its_corners():
    """The corner rule of the tiled kernel and of filter.h's persp_footprint(): over every tile of random valid quads the
    smallest and largest x0 and y0 occur at the four corners."""
    rng = np.random.default_rng(13)
    done = 0
    while done < 60:
        w, h, wo, ho = 96, 80, int(rng.integers(3, 10)) * 16, int(rng.integers(20, 100))
        hh = random_quad_h(rng, w, h, wo, ho)
        if hh is None:
            continue
        done += 1
        Y, X = np.mgrid[0:ho, 0:wo].astype(np.int64)
        x0, y0, _, _ = ref_coord(hh, BILINEAR, X, Y)
        for X0, X1, Y0, Y1 in tiles(wo, ho, 1):
            for X0, X1 in ((X0, X1), (X0, min(X0 + 15, X1))):                    # the 64 x 32 tile and a 16 x 32 part of it
                cx, cy, _, _ = ref_coord(hh, BILINEAR, [X0, X1, X0, X1], [Y0, Y0, Y1, Y1])
                sx, sy = x0[Y0:Y1 + 1, X0:X1 + 1], y0[Y0:Y1 + 1, X0:X1 + 1]
                assert sx.min() == cx.min() and sx.max() == cx.max() and sy.min() == cy.min() and sy.max() == cy.max(), (hh, X0, X1, Y0, Y1)
                b = box(hh, CLAMP, w, h, X0, X1, Y0, Y1)
                assert b[0] <= np.clip(sx, 0, w - 1).min() and np.clip(sx + 1, 0, w - 1).max() <= b[1] and b[2] <= np.clip(sy, 0, h - 1).min() and np.clip(sy + 1, 0, h - 1).max() <= b[3]


def test_error_bound_against_real_valued_bilinear():
    """|exact - real| < 0.5 + 255 * 2^-11 at the exact rational position."""
    img = np.random.default_rng(17).integers(0, 256, size=(1, 80, 96, 3), dtype=np.uint8)
    for name, hh in named_maps(96, 80, 144, 70).items():
        for border in BORDERS:
            err = np.abs(ref_warp(img, hh, 144, 70, BILINEAR, border, 40).astype(np.float64) - float_warp(img, hh, 144, 70, border, 40))
            assert err.max() < 0.5 + 255 * 2.0 ** -11 + 1e-9, (name, border, err.max())


def test_entry_statuses(pkg, L):
    """INVALID before NO_DEVICE, argument for argument as mi_blur_enqueue_warp."""
    ident = affine_h([Q, 0, 0, 0, Q, 0])
    mk = lambda wo=16, ho=16, mode=BILINEAR, border=CONSTANT, fill=0, h=None: make_persp(pkg, h or ident, wo, ho, mode, border, fill)
    horizon = [Q, 0, 0, 0, Q, 0, -Q // 8, 0, Q]                                        # D = 0 at X = 8
    over = list(ident)
    over[5] = OFF_MAX + 1
    own = [(C.byref(mk(h=hh)),) for hh in (over, horizon, [Q, 0, 0, 0, Q, 0, 0, 0, 0])]
    good, rows = (C.byref(mk()),), size_rows(mk) + sampler_rows(mk) + [(8, 8, 3, args) for args in own]
    a, b = check_cpu_run_refuses(PERSP, pkg, L, good, rows)
    check_enqueue_invalid_before_no_device(PERSP, pkg, L, good, rows)
    assert L.mi_blur_cpu_run_warp_perspective(a.ctypes.data, b.ctypes.data, 8, 8, 3, 1, C.byref(mk(h=horizon, wo=8)), 1) == pkg.OK   # the same map, an output that ends before the horizon
    bad = [dict(wo=0), dict(ho=0), dict(wo=MAX_DIM + 1, ho=1), dict(wo=1, ho=MAX_DIM + 1), dict(mode=2), dict(border=2), dict(fill=256), dict(fill=-1)]
    check_ctx_set_refuses(PERSP, pkg, L, good, [(C.byref(mk(**kw)),) for kw in bad] + own + [(C.byref(mk(MAX_DIM, MAX_DIM)),)])


@pytest.mark.parametrize("target", [(42, 37), (63, 74)], ids=lambda t: "x".join(map(str, t)))
def test_cpu_context(pkg, L, target):
    img = np.random.default_rng(23).integers(0, 256, size=(5, 37, 42, 3), dtype=np.uint8)
    n, h, w, c = img.shape
    wo, ho = target
    hh = named_maps(w, h, wo, ho)["tilt"]
    for mode in MODES:
        for border in BORDERS:
            check_cpu_context(PERSP, pkg, L, img, (hh, wo, ho, mode, border, 33))


def test_setters_replace_each_other(pkg, L):
    img = np.random.default_rng(29).integers(0, 256, size=(2, 20, 24, 3), dtype=np.uint8)
    n, h, w, c = img.shape
    hh = named_maps(w, h, 40, 31)["keystone"]
    m = rotation_m(w, h, -40.0)

    persp = lambda ctx: ctx.set_warp_perspective(make_persp(pkg, hh, 40, 31, BILINEAR, CLAMP))
    affine = lambda ctx: ctx.set_warp(make_warp(pkg, m, 30, 11, BILINEAR, CLAMP))
    median = lambda ctx: ctx.set_median(1)
    key, rot, med = ref_warp(img, hh, 40, 31, BILINEAR, CLAMP), ref_affine(img, m, 30, 11, BILINEAR, CLAMP), cpu_run_same_size(MEDIAN, pkg, L, img, 1, 1)
    check_setters_replace_each_other(pkg, L, img, [([persp, median], med), ([median, persp], key), ([persp, affine], rot), ([affine, persp], key)])   # the last one wins


def test_numpy_functions_on_the_cpu_device(pkg, L):
    rng = np.random.default_rng(31)
    stack = rng.integers(0, 256, size=(4, 45, 71, 3), dtype=np.uint8)
    quad = named_quads(71, 45)["tilt"]
    for img in (stack, stack[0], np.ascontiguousarray(stack[0, :, :, 0])):
        as4 = img if img.ndim == 4 else img[None] if img.ndim == 3 else img[None, :, :, None]
        shape = lambda want: want.reshape(want.shape if img.ndim == 4 else want.shape[1:] if img.ndim == 3 else want.shape[1:3])
        for dsize in (None, (100, 33)):
            wo, ho = dsize or (71, 45)
            M = pkg.perspective_matrix(quad, out_corners(wo, ho))
            hh = set_matrix([v for row in M for v in row], False, wo, ho)[0]
            for mode, mo in (("bilinear", BILINEAR), ("nearest", NEAREST)):
                for border, bo in (("constant", CONSTANT), ("clamp", CLAMP)):
                    got = pkg.warp_perspective(img, M, dsize, mode, border, 9, device=pkg.DEVICE_CPU, batch=3)
                    want = shape(ref_warp(as4, hh, wo, ho, mo, bo, 9))
                    assert got.shape == want.shape and got.ndim == img.ndim and np.array_equal(got, want), (img.ndim, dsize, mode, border)
    inv = [1.0, 0.1, -3.0, 0.05, 0.9, 2.0, 1e-4, -2e-4, 1.0]
    assert np.array_equal(pkg.warp_perspective(stack, np.array(inv).reshape(3, 3), inverse=True, device=pkg.DEVICE_CPU),
                          ref_warp(stack, set_matrix(inv, True, 71, 45)[0], 71, 45))          # bilinear, constant 0 by default
    empty = pkg.warp_perspective(np.zeros((0, 45, 71, 3), np.uint8), M, (10, 20), device=pkg.DEVICE_CPU)
    assert empty.shape == (0, 20, 10, 3) and empty.dtype == np.uint8
    for bad in (dict(mode="cubic"), dict(border="reflect"), dict(dsize=(0, 20)), dict(fill=256)):
        with pytest.raises(ValueError):
            pkg.warp_perspective(stack, M, device=pkg.DEVICE_CPU, **bad)
    with pytest.raises(ValueError):
        pkg.warp_perspective(stack, [[1, 0, 0], [0, 1, 0]], device=pkg.DEVICE_CPU)
    with pytest.raises(pkg.MiBlurError):
        pkg.warp_perspective(stack, [[1, 2, 3], [2, 4, 6], [0, 0, 1]], device=pkg.DEVICE_CPU)      # singular
    with pytest.raises(pkg.MiBlurError):
        pkg.warp_perspective(stack, [[1, 0, 0], [0, 1, 0], [-1.0 / 30, 0, 1]], inverse=True, device=pkg.DEVICE_CPU)   # the horizon at X = 30


def test_hosts_and_the_perspective_option(pkg, tmp_path):
    from resample_harness import read_ppm, write_ppm
    pkg.build_native()
    het, split = os.path.join(pkg.APPS, "heterogeneous_blur"), os.path.join(pkg.APPS, "split_image_blur")
    quad = named_quads(64, 48)["keystone"]
    arg = ",".join(repr(float(v)) for p in quad for v in p)
    base = ["cpu", "0", "35", "--size", "32x24", "--images", "4", "--perspective", arg]
    for extra in (["--sigma", "1.0"], ["--median", "3"], ["--erode", "3"], ["--bilateral", "5"], ["--conv", "sobel"], ["--pyr-down"], ["--ksize", "5"],
                  ["--resize", "64x48"], ["--rotate", "30"], ["--resident"], ["--frames", str(tmp_path)]):
        r = subprocess.run([het, *base, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Error: --perspective excludes" in r.stdout, extra
    for bad in ("1,2,3", "abc", arg + ",5", arg + "x"):
        r = subprocess.run([het, "cpu", "0", "35", "--size", "32x24", "--images", "4", "--perspective", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Error: --perspective x0,y0" in r.stdout, bad
    r = subprocess.run([split, "0.5", "35", "--size", "32x24", "--images", "4", "--perspective", arg], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--perspective" in r.stdout and "bands are not supported" in r.stdout
    img = np.random.default_rng(19).integers(0, 256, size=(48, 64, 3), dtype=np.uint8)
    src = tmp_path / "in.ppm"
    write_ppm(src, img)
    hh = quad_h(64, 48, 64, 48, quad)
    for flags, mode, border, fill, name in (([], BILINEAR, CLAMP, 0, "bilinear"), (["--nearest", "--border-fill", "77"], NEAREST, CONSTANT, 77, "nearest")):
        dst = tmp_path / f"{name}.ppm"
        r = subprocess.run([het, "cpu", "0", "35", "--image", str(src), "--images", "4", "--perspective", arg, *flags, "--save", str(dst)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert f"Blur kernel: {name} warp, perspective, 64x48 -> 64x48" in r.stdout
        assert np.array_equal(read_ppm(dst), ref_warp(img[None], hh, 64, 48, mode, border, fill)[0]), name
    # a quad whose horizon crosses the output (a bow tie), and one with three corners in line: messages, not crashes
    for bad in ("0,0,63,47,63,0,0,47", "0,0,30,0,60,0,0,47"):
        r = subprocess.run([het, "cpu", "0", "35", "--image", str(src), "--images", "4", "--perspective", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode not in (0, -6, -11, 134, 139) and "Error: --perspective:" in r.stdout, (bad, r.stdout[-500:])


@needs_gxx
def test_cpu_device_and_tile_walk_clean_under_asan_ubsan(pkg, tmp_path):
    """tests/san_warp_perspective.cpp: the CPU device against a plain restatement in exact-size heap buffers, and every
    warp_tap offset of every tile of the named, limit and extreme cases against the LDS size the host walk returns."""
    lines = []                                                                   # the named maps need the setter: handed over as data
    for (n, h, w, c), (wo, ho) in TILED_SHAPES:
        lines += [" ".join(map(str, [w, h, c, wo, ho] + hh)) for hh in named_maps(w, h, wo, ho).values()]
    lines.append(" ".join(map(str, [512, 512, 1, 128, 128] + quad_h(512, 512, 128, 128, BIG_QUAD))))
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    run_sanitized(pkg, tmp_path, ("san_warp_perspective.cpp", "cpu_device.cpp"), ["perspective warp cases clean", "taps inside their LDS"], [cases])
