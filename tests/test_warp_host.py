"""The affine warp (mi_blur_warp_coord, mi_blur_warp_rotation, mi_blur_warp_set_matrix, mi_blur_cpu_run_warp,
mi_blur_enqueue_warp's argument checks, mi_blur_ctx_set_warp, warp_affine() / rotate() / warp_coord()), CPU only: against
the numpy restatement of the header's definition (warp_ref.py), independent of the product.  All comparisons are exact
unless stated."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from filter_harness import MEDIAN, cpu_run as cpu_run_same_size
from resample_harness import (WARP, check_cpu_context, check_cpu_run_refuses, check_ctx_set_refuses, check_enqueue_invalid_before_no_device,
                              check_setters_replace_each_other, cpu_run, needs_gxx, no_scratch, run_sanitized, sampler_rows, size_rows)
from resize_ref import ref_resize
from warp_ref import (BILINEAR, CLAMP, CONSTANT, EXTREME, LIMIT_FILL, LIMIT_MAPS, LIN_MAX, MAX_DIM, NEAREST, OFF_MAX, Q, corner_pixels,
                      extreme_id, float_warp, identity, in_the_admitted_region, invert, limit_out, limit_references, make_warp, max_footprint,
                      narrow_cases, outside_share, quantise, ref_coord, ref_warp, ref_warp_band, rot90_matrix, rotation_forward, rotation_m,
                      scale_matrix, takes_tiled)

MODES = (BILINEAR, NEAREST)
BORDERS = (CLAMP, CONSTANT)


def shear_m(kx, ky, tx=0.0, ty=0.0):
    return quantise([1.0, kx, tx, ky, 1.0, ty])


def test_coord_equals_the_restatement(pkg, L):
    rng = np.random.default_rng(1)
    x0, y0, fx, fy = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    mats = [identity(), rot90_matrix(17), [0] * 6, [LIN_MAX, -LIN_MAX, OFF_MAX, -LIN_MAX, LIN_MAX, -OFF_MAX], [-LIN_MAX] * 2 + [-OFF_MAX] + [LIN_MAX] * 2 + [OFF_MAX],
            [1, -1, 15, -1, 1, -17], [Q, 0, -16, 0, Q, -17], [Q, 0, 32767, 0, Q, 32768]]
    for _ in range(40):
        lin = rng.integers(-LIN_MAX, LIN_MAX + 1, size=4) if rng.random() < 0.5 else rng.integers(-2 * Q, 2 * Q + 1, size=4)
        off = rng.integers(-OFF_MAX, OFF_MAX + 1, size=2) if rng.random() < 0.5 else rng.integers(-300 * Q, 300 * Q, size=2)
        mats.append([int(lin[0]), int(lin[1]), int(off[0]), int(lin[2]), int(lin[3]), int(off[1])])
    pts = [(0, 0), (1, 0), (0, 1), (13, 7), (MAX_DIM - 1, MAX_DIM - 1), (MAX_DIM - 1, 0)]
    for m in mats:
        for mode in MODES:
            wp = make_warp(pkg, m, 1, 1, mode)
            for X, Y in pts:
                assert L.mi_blur_warp_coord(C.byref(wp), X, Y, C.byref(x0), C.byref(y0), C.byref(fx), C.byref(fy)) == pkg.OK
                want = tuple(int(v) for v in ref_coord(m, mode, X, Y))
                assert (x0.value, y0.value, fx.value, fy.value) == want, (m, mode, X, Y)
                assert 0 <= fx.value <= 2047 and 0 <= fy.value <= 2047 and (mode == BILINEAR or (fx.value, fy.value) == (0, 0))
                assert pkg.warp_coord(wp, X, Y) == want
    good = make_warp(pkg, identity(), 1, 1)
    for X, Y in ((-1, 0), (0, -1), (MAX_DIM, 0), (0, MAX_DIM)):
        assert L.mi_blur_warp_coord(C.byref(good), X, Y, C.byref(x0), C.byref(y0), C.byref(fx), C.byref(fy)) == pkg.ERR_INVALID
    assert L.mi_blur_warp_coord(None, 0, 0, C.byref(x0), C.byref(y0), C.byref(fx), C.byref(fy)) == pkg.ERR_INVALID
    assert L.mi_blur_warp_coord(C.byref(good), 0, 0, None, C.byref(y0), C.byref(fx), C.byref(fy)) == pkg.ERR_INVALID
    assert L.mi_blur_warp_coord(C.byref(make_warp(pkg, identity(), 1, 1, 2)), 0, 0, C.byref(x0), C.byref(y0), C.byref(fx), C.byref(fy)) == pkg.ERR_INVALID
    over = identity()
    over[1] = LIN_MAX + 1
    assert L.mi_blur_warp_coord(C.byref(make_warp(pkg, over, 1, 1)), 0, 0, C.byref(x0), C.byref(y0), C.byref(fx), C.byref(fy)) == pkg.ERR_INVALID


def test_properties_of_the_definition(pkg, L):
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, size=(2, 13, 17, 3), dtype=np.uint8)
    n, h, w, c = img.shape
    for mode in MODES:
        for border in BORDERS:
            run = lambda m, wo, ho, fill=7: cpu_run(WARP, pkg, L, img, (m, wo, ho, mode, border, fill), 2)
            assert np.array_equal(run(identity(), w, h), img)                                      # the identity
            # the four right-angle rotations, each from the header's rot90 matrix composed with itself
            assert np.array_equal(run(rot90_matrix(w), h, w), np.rot90(img, 1, axes=(1, 2)))
            assert np.array_equal(run([-Q, 0, (w - 1) * Q, 0, -Q, (h - 1) * Q], w, h), np.rot90(img, 2, axes=(1, 2)))
            assert np.array_equal(run([0, Q, 0, -Q, 0, (h - 1) * Q], h, w), np.rot90(img, 3, axes=(1, 2)))
            assert np.array_equal(run([Q, 0, 0, 0, Q, 0], w, h), np.rot90(img, 4, axes=(1, 2)))
            # flips and the transpose
            assert np.array_equal(run([-Q, 0, (w - 1) * Q, 0, Q, 0], w, h), img[:, :, ::-1])
            assert np.array_equal(run([Q, 0, 0, 0, -Q, (h - 1) * Q], w, h), img[:, ::-1])
            assert np.array_equal(run([0, Q, 0, Q, 0, 0], h, w), img.transpose(0, 2, 1, 3))
            # integer shifts: output (X, Y) = input (X + dx, Y + dy), the rest by the border rule
            for dx, dy in ((3, 0), (0, -2), (-5, 4), (20, 0), (0, -30)):
                got = run(identity(dx, dy), w, h)
                ys, xs = np.arange(h) + dy, np.arange(w) + dx
                want = img[:, np.clip(ys, 0, h - 1)][:, :, np.clip(xs, 0, w - 1)].copy()
                if border == CONSTANT:
                    want[:, (ys < 0) | (ys >= h)] = 7
                    want[:, :, (xs < 0) | (xs >= w)] = 7
                assert np.array_equal(got, want), (mode, border, dx, dy)
            # a zero linear part samples one position
            got = run([0, 0, 5 * Q, 0, 0, 3 * Q], 9, 4)
            assert (got == img[:, 3:4, 5:6]).all()
    flat = np.full((1, 9, 16, 2), 255, np.uint8)
    for m in (rotation_m(16, 9, 33.0), shear_m(0.4, -0.3, 2.5, -1.25), scale_matrix(2, 1), identity(-40, 3)):
        for mode in MODES:
            assert (cpu_run(WARP, pkg, L, flat, (m, 21, 14, mode, CLAMP, 0), 2) == 255).all()
            assert (cpu_run(WARP, pkg, L, flat, (m, 21, 14, mode, CONSTANT, 255), 2) == 255).all()
            assert (ref_warp(flat, m, 21, 14, mode, CONSTANT, 255) == 255).all()


@pytest.mark.parametrize("ratio", [(2, 1), (4, 1), (1, 2), (1, 4), (1, 8)], ids=lambda r: f"{r[0]}over{r[1]}")
def test_clamp_scale_equals_the_resize(pkg, L, ratio):
    num, den = ratio
    img = np.random.default_rng(3).integers(0, 256, size=(2, 24, 40, 3), dtype=np.uint8)
    wo, ho = 40 * num // den, 24 * num // den
    want = ref_resize(img, wo, ho)
    m = scale_matrix(num, den)
    assert np.array_equal(ref_warp(img, m, wo, ho, BILINEAR, CLAMP), want)
    assert np.array_equal(cpu_run(WARP, pkg, L, img, (m, wo, ho, BILINEAR, CLAMP, 0), 2), want)


@pytest.mark.parametrize("case", ["rot30", "rot-17.3", "rot45x1.3", "shear", "shear2"])
def test_bilinear_is_within_the_bound_of_float_bilinear(pkg, L, case):
    """The header's bound: less than 0.5 + 255 * 2^-11 from real-valued bilinear at the exact Q16 position (each axis
    rounded by at most 2^-12 at slope at most 255, one final rounding), on a 0/255 checkerboard with noise."""
    h, w = 33, 48
    m = {"rot30": rotation_m(w, h, 30.0), "rot-17.3": rotation_m(w, h, -17.3), "rot45x1.3": rotation_m(w, h, 45.0, 1.3),
         "shear": shear_m(0.5, 0.0, -3.3, 1.7), "shear2": shear_m(-0.25, 0.4, 6.1, -2.9)}[case]
    rng = np.random.default_rng(len(case))
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((yy + xx) & 1) * 255).astype(np.int64)[None, :, :, None] + rng.integers(-20, 21, size=(2, h, w, 3))
    img = np.clip(board, 0, 255).astype(np.uint8)
    for border in BORDERS:
        real = float_warp(img, m, 61, 40, border, 90)
        restated = ref_warp(img, m, 61, 40, BILINEAR, border, 90)
        assert np.array_equal(cpu_run(WARP, pkg, L, img, (m, 61, 40, BILINEAR, border, 90), 2), restated)
        assert np.abs(restated.astype(np.float64) - real).max() < 0.5 + 255 * 2.0 ** -11


def cpu_cases(h, w):
    """(m, Wo, Ho): inside, partly outside and wholly outside the input; a reduction; extreme entries."""
    return [(rotation_m(w, h, 30.0), w, h), (rotation_m(w, h, -75.0, 0.7), w + 5, h + 3), (shear_m(0.5, -0.2, -4.5, 3.25), 2 * w + 1, max(1, h // 2)),
            (identity(w + 10, 0), w, h), (identity(-3 * w, -3 * h), 7, 5), (scale_matrix(1, 8), max(1, w // 8), max(1, h // 8)),
            ([LIN_MAX, -LIN_MAX, OFF_MAX, -LIN_MAX, LIN_MAX, -OFF_MAX], 5, 4), ([3, -2, (w - 1) * Q + 65535, 1, 5, -1], 9, 9), (identity(), 1, 1)]


@pytest.mark.parametrize("shape", [(3, 33, 40, 3), (1, 1, 1, 3), (2, 9, 5, 1), (1, 17, 16, 4), (1, 20, 7, 5), (1, 31, 48, 2)], ids=lambda s: "x".join(map(str, s)))
def test_cpu_run_matches_the_restatement(pkg, L, shape):
    img = np.random.default_rng(sum(shape)).integers(0, 256, size=shape, dtype=np.uint8)
    n, h, w, c = shape
    for m, wo, ho in cpu_cases(h, w):
        for mode in MODES:
            for border in BORDERS:
                want = ref_warp(img, m, wo, ho, mode, border, 201)
                assert want.shape == (n, ho, wo, c)
                for nt in (1, 3):
                    assert np.array_equal(cpu_run(WARP, pkg, L, img, (m, wo, ho, mode, border, 201), nt), want), (shape, m, wo, ho, mode, border, nt)


def test_band_reference_equals_the_whole_image_reference():
    """ref_warp_band() against ref_warp() of the whole image: the first band, one in the middle and the last, under a
    sheared map that leaves the image at a corner, both modes and borders.  What the near-2-GiB GPU tests compare with."""
    img = np.random.default_rng(41).integers(0, 256, size=(1, 700, 1024, 3), dtype=np.uint8)
    n, h, w, c = img.shape
    wo, ho, m = 1024, 1399, [Q, 0, 0, 17030, Q // 2, -Q // 4]
    for mode in MODES:
        for border in BORDERS:
            whole = ref_warp(img, m, wo, ho, mode, border, 173)
            assert 0 < outside_share(m, mode, w, h, wo, ho - 8, ho) < 1          # the last band leaves the image in part
            for Y0 in (0, 600, ho - 8):
                got = ref_warp_band(lambda lo, hi: img[:, lo:hi], h, m, wo, Y0, Y0 + 8, mode, border, 173)
                assert np.array_equal(got, whole[:, Y0:Y0 + 8]), (mode, border, Y0)
    # a band wholly below, and one wholly above, the image: the slab is the image's last / first row
    for m2 in ([Q, 0, 0, 0, Q, 800 * Q], [Q, 0, 0, 0, Q, -50 * Q - 7]):
        for border in BORDERS:
            got = ref_warp_band(lambda lo, hi: img[:, lo:hi], h, m2, wo, 16, 24, BILINEAR, border, 173)
            assert np.array_equal(got, ref_warp(img, m2, wo, 24, BILINEAR, border, 173)[:, 16:24]), (m2, border)


def coords_equal_the_restatement(pkg, L, m, wo, ho):
    """mi_blur_warp_coord at the four corner pixels of the output, both modes."""
    for mode in MODES:
        wp = make_warp(pkg, m, wo, ho, mode)
        for X, Y in corner_pixels(wo, ho):
            assert pkg.warp_coord(wp, X, Y) == tuple(int(v) for v in ref_coord(m, mode, X, Y)), (m, mode, X, Y)


@pytest.mark.parametrize("case", EXTREME, ids=extreme_id)
def test_cpu_device_on_extreme_shapes(pkg, L, case):
    """The shapes of test_large_shapes_gpu.py's warp cases: 32768 pixels along one axis, positions up to 2^31."""
    shape, (wo, ho), m, quarter_turns = case
    img = np.random.default_rng(sum(shape)).integers(0, 256, size=(1,) + shape, dtype=np.uint8)
    coords_equal_the_restatement(pkg, L, m, wo, ho)
    for mode in MODES:
        for border in BORDERS:
            want = ref_warp(img, m, wo, ho, mode, border, 173)
            assert np.array_equal(cpu_run(WARP, pkg, L, img, (m, wo, ho, mode, border, 173), 4), want), (mode, border)
            if quarter_turns is not None:
                assert np.array_equal(want, np.rot90(img, quarter_turns, axes=(1, 2)))


def test_cpu_device_on_inputs_of_one_chunk_per_row(pkg, L):
    for img, name, m, wo, ho in narrow_cases():
        coords_equal_the_restatement(pkg, L, m, wo, ho)
        for mode in MODES:
            for border in BORDERS:
                want = ref_warp(img, m, wo, ho, mode, border, 173)
                assert np.array_equal(cpu_run(WARP, pkg, L, img, (m, wo, ho, mode, border, 173), 2), want), (img.shape, name, mode, border)


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_cpu_device_on_maps_at_the_limits_of_the_header(pkg, L, c):
    """LIMIT_MAPS: coefficients of 2^26 and 2^46, zero and rank-one linear parts, steps of 1 / 65536 pixel."""
    img, refs = limit_references(2, c)
    wo, ho = limit_out(c)
    for name, (m, _, _) in LIMIT_MAPS.items():
        coords_equal_the_restatement(pkg, L, m, wo, ho)
        for mode in MODES:
            for border in BORDERS:
                got = cpu_run(WARP, pkg, L, img, (m, wo, ho, mode, border, LIMIT_FILL), 3)
                assert np.array_equal(got, refs[name, mode, border]), (name, mode, border)


def test_set_matrix_and_rotation(pkg, L):
    img = np.random.default_rng(5).integers(0, 256, size=(1, 30, 44, 3), dtype=np.uint8)
    fwd = (C.c_double * 6)()
    for cx, cy, ang, sc in ((21.5, 14.5, 30.0, 1.0), (0.0, 0.0, -17.3, 0.67), (10.0, 40.0, 135.0, 1.5), (21.5, 14.5, 90.0, 1.0)):
        assert L.mi_blur_warp_rotation(cx, cy, ang, sc, fwd) == pkg.OK
        want_fwd = rotation_forward(cx, cy, ang, sc)
        assert np.allclose(list(fwd), want_fwd, rtol=0, atol=1e-9)
        assert np.allclose(pkg.rotation_matrix((cx, cy), ang, sc), [want_fwd[:3], want_fwd[3:]], rtol=0, atol=1e-9)
        a, b = pkg.Warp(44, 30, BILINEAR, CONSTANT, 0), pkg.Warp(44, 30, BILINEAR, CONSTANT, 0)
        assert L.mi_blur_warp_set_matrix(C.byref(a), fwd, 0) == pkg.OK
        inv = invert(list(fwd))
        assert L.mi_blur_warp_set_matrix(C.byref(b), (C.c_double * 6)(*inv), 1) == pkg.OK
        assert max(abs(x - y) for x, y in zip(a.m, b.m)) <= 1              # the same inverse, computed twice in double
        assert max(abs(x - y) for x, y in zip(b.m, quantise(inv))) == 0
        # the forward and the inverse matrix give the same warp (bytes: the library's own inverse against numpy's)
        got_a = cpu_run(WARP, pkg, L, img, (list(a.m), 44, 30, BILINEAR, CONSTANT, 0), 2)
        assert np.array_equal(got_a, ref_warp(img, list(a.m), 44, 30))
        if list(a.m) == list(b.m):
            assert np.array_equal(got_a, cpu_run(WARP, pkg, L, img, (list(b.m), 44, 30, BILINEAR, CONSTANT, 0), 2))
    # a right angle about the centre of a square is exact: np.rot90
    sq = np.random.default_rng(6).integers(0, 256, size=(1, 12, 12, 2), dtype=np.uint8)
    assert np.array_equal(pkg.rotate(sq, 90.0, device=pkg.DEVICE_CPU), np.rot90(sq, 1, axes=(1, 2)))
    assert np.array_equal(pkg.rotate(sq, 180.0, device=pkg.DEVICE_CPU), np.rot90(sq, 2, axes=(1, 2)))
    wp = pkg.Warp(4, 4, BILINEAR, CLAMP, 0)
    keep = (C.c_int64 * 6)(1, 2, 3, 4, 5, 6)
    wp.m = keep
    d6 = lambda *v: (C.c_double * 6)(*v)
    for bad, inverse in ((d6(1, 2, 0, 2, 4, 0), 0), (d6(0, 0, 0, 0, 0, 0), 0), (d6(float("nan"), 0, 0, 0, 1, 0), 1), (d6(1, 0, float("inf"), 0, 1, 0), 1),
                         (d6(1025.0, 0, 0, 0, 1, 0), 1), (d6(1, 0, 2.0 ** 30 + 1, 0, 1, 0), 1), (d6(1e-4, 0, 0, 0, 1e-4, 0), 0), (d6(1, 0, 0, 0, 1, -2.0 ** 31), 1)):
        assert L.mi_blur_warp_set_matrix(C.byref(wp), bad, inverse) == pkg.ERR_INVALID, list(bad)
        assert list(wp.m) == [1, 2, 3, 4, 5, 6]
    assert L.mi_blur_warp_set_matrix(None, d6(1, 0, 0, 0, 1, 0), 1) == pkg.ERR_INVALID
    assert L.mi_blur_warp_set_matrix(C.byref(wp), None, 1) == pkg.ERR_INVALID
    assert L.mi_blur_warp_rotation(0.0, 0.0, 10.0, 1.0, None) == pkg.ERR_INVALID
    assert L.mi_blur_warp_rotation(float("nan"), 0.0, 10.0, 1.0, fwd) == pkg.ERR_INVALID
    assert L.mi_blur_warp_set_matrix(C.byref(wp), d6(1024.0, 0, 2.0 ** 30, 0, -1024.0, -2.0 ** 30), 1) == pkg.OK      # the limits themselves
    assert list(wp.m) == [LIN_MAX, 0, OFF_MAX, 0, -LIN_MAX, -OFF_MAX]


def mk(pkg, wo=16, ho=16, mode=BILINEAR, border=CONSTANT, fill=0, m=None):
    return make_warp(pkg, m or identity(), wo, ho, mode, border, fill)


def bad_rows(pkg):
    """(good, rows) for resample_harness.bad_calls; the warp's own rows: every entry of m one past its limit, either sign."""
    make = lambda **kw: mk(pkg, **kw)
    rows = size_rows(make) + sampler_rows(make)
    for i in range(6):
        lim = OFF_MAX if i % 3 == 2 else LIN_MAX
        for v in (lim + 1, -lim - 1):
            m = identity()
            m[i] = v
            rows.append((8, 8, 3, (C.byref(mk(pkg, m=m)),)))
    return (C.byref(mk(pkg)),), rows


def test_cpu_run_refuses_invalid_arguments(pkg, L):
    a, b = check_cpu_run_refuses(WARP, pkg, L, *bad_rows(pkg))
    lim = make_warp(pkg, [LIN_MAX, -LIN_MAX, -OFF_MAX, 0, 0, OFF_MAX], 16, 16, BILINEAR, CLAMP, 255)      # the limits themselves are valid
    assert L.mi_blur_cpu_run_warp(a.ctypes.data, b.ctypes.data, 8, 8, 3, 1, C.byref(lim), 1) == pkg.OK


def test_enqueue_invalid_comes_before_no_device(pkg, L):
    """Every argument is checked before a device is asked for; without a GPU a good call is ERR_NO_DEVICE (with one, the
    null stream of an empty batch is MI_BLUR_OK)."""
    check_enqueue_invalid_before_no_device(WARP, pkg, L, *bad_rows(pkg))


def test_ctx_set_refuses_invalid_arguments(pkg, L):
    """The table of mi_blur_ctx_set_resize: a null context or struct is ERR_INVALID whatever the state, an invalid struct
    ERR_INVALID before the first submit, anything ERR_STATE after it; a refused set leaves the filter in place."""
    over = identity()
    over[5] = OFF_MAX + 1
    bad = [dict(wo=0), dict(ho=0), dict(wo=MAX_DIM + 1, ho=1), dict(wo=1, ho=MAX_DIM + 1), dict(mode=2), dict(border=2), dict(fill=256), dict(fill=-1), dict(m=over),
           dict(wo=MAX_DIM, ho=MAX_DIM)]
    check_ctx_set_refuses(WARP, pkg, L, (C.byref(mk(pkg)),), [(C.byref(mk(pkg, **kw)),) for kw in bad])


@pytest.mark.parametrize("target", [(42, 37), (63, 74), (25, 22)], ids=lambda t: "x".join(map(str, t)))
def test_cpu_context(pkg, L, target):
    img = np.random.default_rng(23).integers(0, 256, size=(5, 37, 42, 3), dtype=np.uint8)
    n, h, w, c = img.shape
    wo, ho = target
    m = rotation_m(w, h, 25.0, 1.1)
    for mode in MODES:
        for border in BORDERS:
            check_cpu_context(WARP, pkg, L, img, (m, wo, ho, mode, border, 33))


def test_setters_replace_each_other(pkg, L):
    img = np.random.default_rng(29).integers(0, 256, size=(2, 20, 24, 3), dtype=np.uint8)
    n, h, w, c = img.shape
    m = rotation_m(w, h, -40.0)

    warp = lambda ctx: ctx.set_warp(make_warp(pkg, m, 40, 31, BILINEAR, CLAMP))
    median = lambda ctx: ctx.set_median(1)
    resize = lambda ctx: ctx.set_resize(30, 11)
    rot, med, small = ref_warp(img, m, 40, 31, BILINEAR, CLAMP), cpu_run_same_size(MEDIAN, pkg, L, img, 1, 1), ref_resize(img, 30, 11)
    check_setters_replace_each_other(pkg, L, img, [([warp, median], med), ([median, warp], rot), ([warp, resize], small), ([resize, warp], rot)])   # the last one wins


def test_numpy_functions_on_the_cpu_device(pkg, L):
    rng = np.random.default_rng(31)
    stack = rng.integers(0, 256, size=(4, 45, 71, 3), dtype=np.uint8)
    fwd = rotation_forward(20.0, 10.0, 33.0, 0.9)
    M = [fwd[:3], fwd[3:]]
    m = quantise(invert(fwd))
    for img in (stack, stack[0], np.ascontiguousarray(stack[0, :, :, 0])):
        as4 = img if img.ndim == 4 else img[None] if img.ndim == 3 else img[None, :, :, None]
        shape = lambda want: want.reshape(want.shape if img.ndim == 4 else want.shape[1:] if img.ndim == 3 else want.shape[1:3])
        for dsize in (None, (100, 33)):
            wo, ho = dsize or (71, 45)
            for mode, mo in (("bilinear", BILINEAR), ("nearest", NEAREST)):
                for border, bo in (("constant", CONSTANT), ("clamp", CLAMP)):
                    got = pkg.warp_affine(img, M, dsize, mode, border, 9, device=pkg.DEVICE_CPU, batch=3)
                    want = shape(ref_warp(as4, m, wo, ho, mo, bo, 9))
                    assert got.shape == want.shape and got.ndim == img.ndim and np.array_equal(got, want), (img.ndim, dsize, mode, border)
    inv = invert(fwd)
    assert np.array_equal(pkg.warp_affine(stack, [inv[:3], inv[3:]], inverse=True, device=pkg.DEVICE_CPU), ref_warp(stack, quantise(inv), 71, 45))
    assert np.array_equal(pkg.warp_affine(stack, np.array(M), device=pkg.DEVICE_CPU), ref_warp(stack, m, 71, 45))          # bilinear, constant 0 by default
    assert np.array_equal(pkg.rotate(stack, 30.0, device=pkg.DEVICE_CPU), ref_warp(stack, rotation_m(71, 45, 30.0), 71, 45))  # about the centre
    assert np.array_equal(pkg.rotate(stack[0], -12.5, 1.2, (3.0, 4.0), (50, 60), "nearest", "clamp", device=pkg.DEVICE_CPU),
                          ref_warp(stack[:1], rotation_m(71, 45, -12.5, 1.2, (3.0, 4.0)), 50, 60, NEAREST, CLAMP)[0])
    empty = pkg.warp_affine(np.zeros((0, 45, 71, 3), np.uint8), M, (10, 20), device=pkg.DEVICE_CPU)
    assert empty.shape == (0, 20, 10, 3) and empty.dtype == np.uint8
    for bad in (dict(mode="cubic"), dict(border="reflect"), dict(dsize=(0, 20)), dict(fill=256)):
        with pytest.raises(ValueError):
            pkg.warp_affine(stack, M, device=pkg.DEVICE_CPU, **bad)
    with pytest.raises(ValueError):
        pkg.warp_affine(stack, [[1, 0, 0]], device=pkg.DEVICE_CPU)
    with pytest.raises(ValueError):
        pkg.warp_affine(stack.astype(np.float32), M, device=pkg.DEVICE_CPU)
    with pytest.raises(pkg.MiBlurError):
        pkg.warp_affine(stack, [[1, 2, 0], [2, 4, 0]], device=pkg.DEVICE_CPU)      # singular
    with pytest.raises(pkg.MiBlurError):
        pkg.warp_affine(stack, M, (MAX_DIM + 1, 20), device=pkg.DEVICE_CPU)


def test_the_admitted_region_fits_the_lds():
    """The header's claim, through the restated walk: aligned BILINEAR launches with |m0|+|m1| <= 3Q/2 and |m3|+|m4| <= 3Q/2
    take the tiled kernel (rotations, enlargements, shears to 0.5, the corners of the region), within 98 rows x 27 chunks."""
    mats = [rotation_m(256, 192, a) for a in (0, 30, 45, 90, -17.3, 135)] + [scale_matrix(2, 1), scale_matrix(4, 1), shear_m(0.5, 0.5), shear_m(-0.5, 0.5, 9.5, -3.25)]
    mats += [[3 * Q // 2, 0, 0, 0, 3 * Q // 2, 0], [0, -3 * Q // 2, 255 * Q, 3 * Q // 2, 0, 0], [3 * Q // 4, 3 * Q // 4, 11, -3 * Q // 4, 3 * Q // 4, 100 * Q + 7]]
    for m in mats:
        assert in_the_admitted_region(m), m
        for c in (1, 2, 3, 4):
            for border in BORDERS:
                shape = (1, 192, 256, c)
                assert max_footprint(shape, m, 272, 200, border) <= 98 * 27 * 16
                assert takes_tiled(shape, m, 272, 200, BILINEAR, border)
    assert not takes_tiled((1, 512, 512, 1), scale_matrix(1, 8), 64, 64, BILINEAR, CLAMP)         # 512 x 256 pixels under one tile
    assert not takes_tiled((1, 192, 256, 3), rotation_m(256, 192, 30), 272, 200, NEAREST)
    assert not takes_tiled((1, 192, 256, 5), rotation_m(256, 192, 30), 272, 200)


def test_hosts_refuse_rotate_with_other_filters(pkg, tmp_path):
    """The command lines are refused while the flags are parsed, before any device is asked for."""
    pkg.build_native()
    het, split = os.path.join(pkg.APPS, "heterogeneous_blur"), os.path.join(pkg.APPS, "split_image_blur")
    base = ["cpu", "0", "35", "--size", "32x24", "--images", "4", "--rotate", "30"]
    for extra in (["--sigma", "1.0"], ["--median", "3"], ["--erode", "3"], ["--dilate", "3"], ["--morph-gradient", "3"], ["--bilateral", "5"],
                  ["--conv", "sobel"], ["--pyr-down"], ["--ksize", "5"], ["--resize", "64x48"], ["--resident"], ["--frames", str(tmp_path)]):
        r = subprocess.run([het, *base, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Error: --rotate excludes" in r.stdout, extra
    r = subprocess.run([het, "cpu", "0", "35", "--size", "32x24", "--images", "4", "--border-fill", "9"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Error: --border-fill needs --rotate" in r.stdout
    r = subprocess.run([het, "cpu", "0", "35", "--size", "32x24", "--images", "4", "--nearest"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Error: --nearest needs --resize" in r.stdout
    for bad in (["--rotate", "abc"], ["--rotate", "30x"], ["--rotate", "30", "--border-fill", "256"], ["--rotate", "30", "--border-fill", "-1"]):
        r = subprocess.run([het, "cpu", "0", "35", "--size", "32x24", "--images", "4", *bad], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and ("Error: --rotate DEG" in r.stdout or "Error: --border-fill V" in r.stdout), bad
    r = subprocess.run([split, "0.5", "35", "--size", "32x24", "--images", "4", "--rotate", "30"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--rotate" in r.stdout and "bands are not supported" in r.stdout


def test_host_rotates_on_the_cpu_device(pkg, tmp_path):
    from resample_harness import read_ppm, write_ppm
    pkg.build_native()
    het = os.path.join(pkg.APPS, "heterogeneous_blur")
    img = np.random.default_rng(19).integers(0, 256, size=(48, 64, 3), dtype=np.uint8)
    src = tmp_path / "in.ppm"
    write_ppm(src, img)
    for flags, mode, border, fill, name in (([], BILINEAR, CLAMP, 0, "bilinear"), (["--nearest", "--border-fill", "77"], NEAREST, CONSTANT, 77, "nearest")):
        dst = tmp_path / f"{name}.ppm"
        r = subprocess.run([het, "cpu", "0", "35", "--image", str(src), "--images", "4", "--rotate", "30", *flags, "--save", str(dst)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert f"Blur kernel: {name} warp, rotate 30 deg, 64x48 -> 64x48" in r.stdout
        assert np.array_equal(read_ppm(dst), ref_warp(img[None], rotation_m(64, 48, 30.0), 64, 48, mode, border, fill)[0]), name


def test_tiled_kernels_use_no_scratch(pkg, tmp_path):
    """Compiles warp_kernels.hip to gfx950 assembly (no GPU needed): the taps are read from LDS at run-time addresses, but
    no tiled instantiation may spill or index registers at run time."""
    no_scratch(pkg, tmp_path, "warp_kernels.hip", "blur_warp_tiled_kernel", 4, dynamic_lds_only=True)       # 1-4 channels; all LDS is sized per launch


@needs_gxx
def test_cpu_warp_clean_under_asan_ubsan(pkg, tmp_path):
    run_sanitized(pkg, tmp_path, ("san_warp.cpp", "cpu_device.cpp"), ["random and edge warp cases clean"])


@needs_gxx
def test_tile_geometry_stays_inside_the_lds_under_asan_ubsan(pkg, tmp_path):
    """The footprint and tap arithmetic the resize and warp tiled kernels share with their host-side LDS sizing
    (filter.h), walked tile by tile on the CPU: tests/san_tile_bounds.cpp."""
    run_sanitized(pkg, tmp_path, ("san_tile_bounds.cpp",), ["taps inside their LDS"])
