"""The remap (mi_blur_remap_coord, mi_blur_remap_from_float, mi_blur_remap_undistort, mi_blur_remap_plan,
mi_blur_cpu_run_remap, mi_blur_enqueue_remap's argument checks, mi_blur_ctx_set_remap, remap() / undistort() and the
hosts' --undistort), CPU only: against the numpy restatement of the header's definition (remap_ref.py), independent of
the product, and against the two oracles already in the tree: every affine and perspective warp is a remap whose map
came from mi_blur_warp_coord / mi_blur_warp_perspective_coord.  All comparisons are exact unless stated."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import warp_perspective_ref as pr
import warp_ref as wr
from filter_harness import MEDIAN, cpu_run as cpu_run_same_size
from remap_ref import (BARREL_DIST, BILINEAR, CLAMP, CONSTANT, I32_MAX, I32_MIN, MAX_DIM, MIXED_SHAPE, NEAREST, ONE, QUANT_LIMIT, STAGE_MAX,
                       abi_affine_map, abi_perspective_map, affine_map, barrel_K, build_map, extreme_entries, float_remap, identity_map,
                       make_remap, mixed_map, quantise, ref_coord, ref_plan, ref_remap, ref_undistort, ref_undistort_real)
from resample_harness import (PERSP, REMAP, WARP, check_cpu_context, check_cpu_run_refuses, check_ctx_set_refuses, check_enqueue_invalid_before_no_device,
                              check_setters_replace_each_other, cpu_run, needs_gxx, no_scratch, run_sanitized, sampler_rows, size_rows)
from resize_ref import ref_resize

MODES = (BILINEAR, NEAREST)
BORDERS = (CLAMP, CONSTANT)


def wild(rng, w, h, wo, ho):
    return np.stack([rng.integers(-3 * ONE, (w + 2) * ONE + 1, size=(ho, wo)), rng.integers(-3 * ONE, (h + 2) * ONE + 1, size=(ho, wo))], axis=-1).astype(np.int32)


@pytest.mark.parametrize("c", [1, 2, 3, 5])
def test_cpu_device_equals_the_restatement(pkg, L, c):
    """Both modes, both borders, one and three images, odd shapes, a 1 x 1 input and a 1 x 1 output; the guard bytes either
    side of the output are checked inside cpu_run."""
    rng = np.random.default_rng(40 + c)
    for (h, w), (wo, ho) in (((17, 33), (48, 29)), ((1, 1), (9, 7)), ((17, 33), (1, 1))):
        for n in (1, 3):
            img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
            for fmap in (wild(rng, w, h, wo, ho), build_map("barrel", w, h, wo, ho), build_map("extremes", w, h, wo, ho)):
                for mode in MODES:
                    for border in BORDERS:
                        got = cpu_run(REMAP, pkg, L, img, (fmap, mode, border, 201, 0), 3)
                        assert np.array_equal(got, ref_remap(img, fmap, mode, border, 201)), (h, w, wo, ho, n, mode, border)


def test_the_identity_map(pkg, L):
    img = np.random.default_rng(2).integers(0, 256, size=(2, 13, 17, 3), dtype=np.uint8)
    for mode in MODES:
        for border in BORDERS:
            assert np.array_equal(cpu_run(REMAP, pkg, L, img, (identity_map(17, 13), mode, border, 7, 0), 2), img)


def far_right(w):
    return wr.identity(w + 70, 0)


@pytest.mark.parametrize("name", ["rot30", "shear0.5", "scale1.5", "far-right", "half-out"])
def test_maps_from_warp_coord_give_the_warp(pkg, L, name):
    """px = clip(x0 * 2048 + fx) with x0, fx from mi_blur_warp_coord itself: the bytes of mi_blur_cpu_run_warp, both borders."""
    img = np.random.default_rng(5).integers(0, 256, size=(2, 20, 24, 3), dtype=np.uint8)
    n, h, w, c = img.shape
    wo, ho = 31, 22
    m = {"rot30": wr.rotation_m(w, h, 30.0), "shear0.5": wr.quantise([1.0, 0.5, -20.75, -0.5, 1.0, 30.5]), "scale1.5": wr.quantise([1.5, 0, -7.25, 0, 1.5, 3.5]),
         "far-right": far_right(w), "half-out": wr.rotation_m(w, h, 20.0, 1.0, (0.0, 0.0))}[name]
    fmap = abi_affine_map(pkg, L, m, wo, ho)
    assert np.array_equal(fmap, affine_map(m, wo, ho))                      # the numpy builder the GPU tests use is the same map
    for border in BORDERS:
        want = cpu_run(WARP, pkg, L, img, (m, wo, ho, BILINEAR, border, 99), 2)
        assert np.array_equal(cpu_run(REMAP, pkg, L, img, (fmap, BILINEAR, border, 99, 0), 2), want), border
        assert np.array_equal(ref_remap(img, fmap, BILINEAR, border, 99), want), border


def test_a_map_from_warp_perspective_coord_gives_the_perspective_warp(pkg, L):
    img = np.random.default_rng(6).integers(0, 256, size=(2, 20, 24, 3), dtype=np.uint8)
    n, h, w, c = img.shape
    wo, ho = 31, 22
    hm = pr.named_maps(w, h, wo, ho)["keystone"]
    fmap = abi_perspective_map(pkg, L, hm, wo, ho)
    for border in BORDERS:
        want = cpu_run(PERSP, pkg, L, img, (hm, wo, ho, BILINEAR, border, 99), 2)
        assert np.array_equal(cpu_run(REMAP, pkg, L, img, (fmap, BILINEAR, border, 99, 0), 2), want), border


@pytest.mark.parametrize("ratio", [(2, 1), (4, 1), (1, 2), (1, 4), (1, 8)], ids=lambda r: f"{r[0]}over{r[1]}")
def test_clamp_scale_maps_give_the_resize(pkg, L, ratio):
    num, den = ratio
    img = np.random.default_rng(3).integers(0, 256, size=(2, 24, 40, 3), dtype=np.uint8)
    wo, ho = 40 * num // den, 24 * num // den
    fmap = affine_map(wr.scale_matrix(num, den), wo, ho)
    want = ref_resize(img, wo, ho)
    assert np.array_equal(cpu_run(REMAP, pkg, L, img, (fmap, BILINEAR, CLAMP, 0, 0), 2), want)
    if ratio == (2, 1):
        assert np.array_equal(pkg.resize(img, (wo, ho), device=pkg.DEVICE_CPU), want)


def test_extreme_entries_give_the_nearest_position_in_range(pkg, L):
    """INT32_MIN, INT32_MAX, -4097 and (W + 1) * 2048 + 1, in x, in y and in both: the bytes of the clamped position."""
    img = np.random.default_rng(7).integers(0, 256, size=(2, 9, 12, 2), dtype=np.uint8)
    n, h, w, c = img.shape
    ex, ey = extreme_entries(w), [I32_MIN, I32_MAX, -4097, (h + 1) * ONE + 1]
    base = identity_map(8, 6, 700, 300)
    raw, near = base.copy(), base.copy()
    k = 0
    for vx, vy in [(x, None) for x in ex] + [(None, y) for y in ey] + list(zip(ex, ey[::-1])):
        Y, X = divmod(k * 3 + 1, 8)
        k += 1
        if vx is not None:
            raw[Y, X, 0], near[Y, X, 0] = vx, min(max(vx, -2 * ONE), (w + 1) * ONE)
        if vy is not None:
            raw[Y, X, 1], near[Y, X, 1] = vy, min(max(vy, -2 * ONE), (h + 1) * ONE)
    assert (raw != near).sum() == 16
    for mode in MODES:
        for border in BORDERS:
            got = cpu_run(REMAP, pkg, L, img, (raw, mode, border, 44, 0), 2)
            assert np.array_equal(got, cpu_run(REMAP, pkg, L, img, (near, mode, border, 44, 0), 2)), (mode, border)
            assert np.array_equal(got, ref_remap(img, raw, mode, border, 44)), (mode, border)


def test_coord_equals_the_restatement(pkg, L):
    x0, y0, fx, fy = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    for w, h in ((1, 1), (17, 33), (MAX_DIM, MAX_DIM)):
        grid = sorted({I32_MIN, I32_MAX, -4097, -4096, -4095, -2049, -2048, -2047, -1025, -1024, -1023, -1, 0, 1, 1023, 1024, 1025, 2047, 2048,
                       (w - 1) * ONE, w * ONE - 1, w * ONE, (w + 1) * ONE - 1, (w + 1) * ONE, (w + 1) * ONE + 1, (h + 1) * ONE, (h + 1) * ONE + 1})
        for mode in MODES:
            r = make_remap(pkg, 1, 1, mode)
            for px in grid:
                for py in (grid[0], grid[-1], -4097, 0, 1024, 1535, (h + 1) * ONE, (h + 1) * ONE + 1):
                    assert L.mi_blur_remap_coord(C.byref(r), w, h, px, py, C.byref(x0), C.byref(y0), C.byref(fx), C.byref(fy)) == pkg.OK
                    want = tuple(int(v) for v in ref_coord(px, py, mode, w, h))
                    assert (x0.value, y0.value, fx.value, fy.value) == want, (w, h, mode, px, py)
                    assert -2 <= x0.value <= w + 1 and -2 <= y0.value <= h + 1 and 0 <= fx.value <= 2047 and 0 <= fy.value <= 2047
                    assert pkg.remap_coord(w, h, px, py, mode) == want
    good = make_remap(pkg, 1, 1)
    out = (C.byref(x0), C.byref(y0), C.byref(fx), C.byref(fy))
    assert L.mi_blur_remap_coord(None, 4, 4, 0, 0, *out) == pkg.ERR_INVALID
    assert L.mi_blur_remap_coord(C.byref(good), 4, 4, 0, 0, None, *out[1:]) == pkg.ERR_INVALID
    assert L.mi_blur_remap_coord(C.byref(make_remap(pkg, 1, 1, 2)), 4, 4, 0, 0, *out) == pkg.ERR_INVALID
    for w, h in ((0, 4), (4, 0), (MAX_DIM + 1, 4), (4, MAX_DIM + 1)):
        assert L.mi_blur_remap_coord(C.byref(good), w, h, 0, 0, *out) == pkg.ERR_INVALID


def test_from_float(pkg, L):
    # exact on dyadic inputs; half a unit rounds up, also below zero; the clamp at +-2^30
    xs = np.array([[0.0, 1.0, -1.0, 3.5, 100.25, -7.125, 1 / 2048, -1 / 2048]], np.float32)
    ys = np.array([[0.5 / 2048, 1.5 / 2048, -0.5 / 2048, -1.5 / 2048, 2.5 / 2048, 0.49 / 2048, 1e9, -1e9]], np.float32)
    got = pkg.remap_map(xs, ys)
    assert got.dtype == np.int32 and got.shape == (1, 8, 2)
    assert got[0, :, 0].tolist() == [0, 2048, -2048, 7168, 205312, -14592, 1, -1]
    assert got[0, :, 1].tolist() == [1, 2, 0, -1, 3, 0, QUANT_LIMIT, -QUANT_LIMIT]
    assert np.array_equal(got, quantise(xs, ys))
    rng = np.random.default_rng(8)
    xs, ys = (rng.uniform(-50, 700, size=(23, 31)).astype(np.float32) for _ in range(2))
    assert np.array_equal(pkg.remap_map(xs, ys), quantise(xs, ys))
    # not finite: INVALID, the destination untouched
    for bad in (np.nan, np.inf, -np.inf):
        for which in (0, 1):
            x, y = np.zeros(6, np.float32), np.ones(6, np.float32)
            (x, y)[which][4] = bad
            dst = np.full(12, 0x5A5A5A5A, np.int32)
            assert L.mi_blur_remap_from_float(x.ctypes.data, y.ctypes.data, 6, dst.ctypes.data) == pkg.ERR_INVALID
            assert (dst == 0x5A5A5A5A).all()
    x = np.zeros(2, np.float32)
    dst = np.zeros(4, np.int32)
    assert L.mi_blur_remap_from_float(None, x.ctypes.data, 2, dst.ctypes.data) == pkg.ERR_INVALID
    assert L.mi_blur_remap_from_float(x.ctypes.data, None, 2, dst.ctypes.data) == pkg.ERR_INVALID
    assert L.mi_blur_remap_from_float(x.ctypes.data, x.ctypes.data, 2, None) == pkg.ERR_INVALID
    assert L.mi_blur_remap_from_float(x.ctypes.data, x.ctypes.data, 0, dst.ctypes.data) == pkg.OK
    with pytest.raises(ValueError):
        pkg.remap_map(np.zeros((3, 4)), np.zeros((4, 3)))


def test_undistort(pkg, L):
    # zero distortion, integer K: the identity grid, exactly
    K = (64.0, 48.0, 31.0, 20.0)
    assert np.array_equal(pkg.undistort_map(K, [0, 0, 0, 0, 0], (40, 30)), identity_map(40, 30))
    assert np.array_equal(pkg.undistort_map(np.array([[64.0, 0, 31.0], [0, 48.0, 20.0], [0, 0, 1]]), [], (40, 30)), identity_map(40, 30))
    # zero distortion, new_K a dyadic scale of K: the exact scaled grid.  new = K / 4 about the origin: u = 4 X, v = 4 Y;
    # new = 2 K: u = X / 2, exact in 11 bits
    Y, X = np.mgrid[0:30, 0:40].astype(np.int64)
    assert np.array_equal(pkg.undistort_map(K, [0] * 5, (40, 30), (16.0, 12.0, 7.75, 5.0)), np.stack([X * 4 * ONE, Y * 4 * ONE], axis=-1))
    assert np.array_equal(pkg.undistort_map(K, [0] * 5, (40, 30), (128.0, 96.0, 62.0, 40.0)), np.stack([X * ONE // 2, Y * ONE // 2], axis=-1))
    # the header's example coefficients on 96 x 80: within one unit of the float64 restatement everywhere (two correct double
    # evaluations differ only where v * 2048 + 0.5 lies within rounding error of an integer, and then by one)
    K = barrel_K(96, 80)
    got = pkg.undistort_map(K, BARREL_DIST, (96, 80))
    want = ref_undistort(K, BARREL_DIST, (96, 80))
    diff = np.abs(got.astype(np.int64) - want)
    print("undistort: units off the float64 restatement: max", diff.max(), "entries off", int((diff != 0).sum()), "of", diff.size)
    assert diff.max() <= 1
    assert np.abs(got.astype(np.int64) - identity_map(96, 80)).max() > 2 * ONE           # and it does distort: by more than two pixels somewhere
    # INVALID
    dst = np.full((4, 4, 2), 0x5A5A5A5A, np.int32)
    d5, d4 = C.c_double * 5, C.c_double * 4
    good_K, good_d = d4(8.0, 8.0, 2.0, 2.0), d5(0, 0, 0, 0, 0)
    call = lambda k, d, nk, wo=4, ho=4, m=dst.ctypes.data: L.mi_blur_remap_undistort(k, d, nk, wo, ho, m)
    assert call(good_K, good_d, None) == pkg.OK
    dst[:] = 0x5A5A5A5A
    for args in [(None, good_d, None), (good_K, None, None), (good_K, good_d, None, 4, 4, None), (good_K, good_d, None, 0, 4), (good_K, good_d, None, 4, MAX_DIM + 1),
                 (d4(0.0, 8.0, 2.0, 2.0), good_d, None), (d4(8.0, 0.0, 2.0, 2.0), good_d, None), (good_K, good_d, d4(0.0, 8.0, 2.0, 2.0)), (good_K, good_d, d4(8.0, 0.0, 2.0, 2.0)),
                 (d4(np.nan, 8.0, 2.0, 2.0), good_d, None), (d4(8.0, 8.0, np.inf, 2.0), good_d, None), (good_K, d5(0, np.nan, 0, 0, 0), None),
                 (good_K, d5(0, 0, 0, 0, -np.inf), None), (good_K, good_d, d4(8.0, 8.0, 2.0, np.nan))]:
        assert call(*args) == pkg.ERR_INVALID, args
    assert (dst == 0x5A5A5A5A).all()
    assert call(d4(0.0, 0.0, 2.0, 2.0), good_d, good_K) == pkg.OK                           # only fx', fy' divide


@pytest.mark.parametrize("border", BORDERS)
def test_bilinear_is_within_the_bound_of_float_bilinear(pkg, L, border):
    """The header's bound, against the REAL positions of the distorted map: less than 0.5 + 255 * 2^-11 (each axis rounded
    by at most 2^-12 at slope at most 255, one final rounding), on a 0/255 checkerboard with noise."""
    h, w = 80, 96
    rng = np.random.default_rng(9)
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((yy + xx) & 1) * 255).astype(np.int64)[None, :, :, None] + rng.integers(-20, 21, size=(2, h, w, 3))
    img = np.clip(board, 0, 255).astype(np.uint8)
    K = barrel_K(w, h)
    u, v = ref_undistort_real(K, BARREL_DIST, (w, h))
    fmap = pkg.undistort_map(K, BARREL_DIST, (w, h))
    real = float_remap(img, u, v, border, 90)
    got = cpu_run(REMAP, pkg, L, img, (fmap, BILINEAR, border, 90, 0), 2).astype(np.float64)
    err = np.abs(got - real).max()
    print("remap against float64 bilinear at the real positions: max error", err)
    assert err < 0.5 + 255 * 2.0 ** -11


def test_plan_equals_the_restated_walk(pkg, L):
    rng = np.random.default_rng(10)
    for c, (wo, ho) in ((1, (144, 70)), (2, (136, 70)), (3, (144, 70)), (4, (132, 70))):
        w, h = 96, 80
        for name in ("rot30", "barrel", "outside", "half-out", "wild", "extremes"):
            fmap = build_map(name, w, h, wo, ho)
            for border in BORDERS:
                for stage in (0, 4096, 16, STAGE_MAX):
                    got = pkg.remap_plan(fmap, w, h, c, "bilinear", border, 0, stage)
                    want = ref_plan(fmap, w, h, c, BILINEAR, border, stage)
                    assert got == want, (c, name, border, stage)
                    assert got["tiled"] == 1 and got["staged"] + got["direct"] + got["empty"] == got["tiles"] == 9
    n, h, w, c = MIXED_SHAPE
    p = pkg.remap_plan(mixed_map(), w, h, c, "bilinear", "clamp")
    assert p == ref_plan(mixed_map(), w, h, c, BILINEAR, CLAMP) and p["staged"] >= 1 and p["direct"] >= 1 and p["max_box_bytes"] > 65536 >= p["max_staged_bytes"]
    out = build_map("outside", 96, 80, 144, 70)
    p = pkg.remap_plan(out, 96, 80, 1, "bilinear", "constant")
    assert p["empty"] == p["tiles"] == 9 and p["max_box_bytes"] == 0
    assert pkg.remap_plan(out, 96, 80, 1, "bilinear", "clamp")["empty"] == 0
    odd = wild(rng, 33, 17, 48, 29)
    zero = dict(tiled=0, tiles=0, staged=0, direct=0, empty=0, max_box_bytes=0, max_staged_bytes=0)
    assert pkg.remap_plan(odd, 33, 17, 3) == zero == ref_plan(odd, 33, 17, 3)                           # odd input rows
    assert pkg.remap_plan(wild(rng, 96, 80, 50, 29), 96, 80, 1) == zero                                # odd output rows
    assert pkg.remap_plan(build_map("rot30", 96, 80, 144, 70), 96, 80, 1, "nearest") == zero
    assert pkg.remap_plan(wild(rng, 64, 24, 128, 48), 64, 24, 5) == zero
    t = pkg.RemapTiles()
    r = make_remap(pkg, 48, 29)
    assert L.mi_blur_remap_plan(None, 33, 17, 3, C.byref(r), C.byref(t)) == pkg.ERR_INVALID
    assert L.mi_blur_remap_plan(odd.ctypes.data, 33, 17, 3, None, C.byref(t)) == pkg.ERR_INVALID
    assert L.mi_blur_remap_plan(odd.ctypes.data, 33, 17, 3, C.byref(r), None) == pkg.ERR_INVALID
    assert L.mi_blur_remap_plan(odd.ctypes.data, 0, 17, 3, C.byref(r), C.byref(t)) == pkg.ERR_INVALID
    assert L.mi_blur_remap_plan(odd.ctypes.data, 33, 17, 3, C.byref(make_remap(pkg, 48, 29, stage_bytes=8)), C.byref(t)) == pkg.ERR_INVALID


# ---------------------------------------------------------------- statuses
def mk(pkg, wo=16, ho=16, mode=BILINEAR, border=CONSTANT, fill=0, stage=0):
    return make_remap(pkg, wo, ho, mode, border, fill, stage)


def bad_rows(pkg, fmap):
    """(good, rows) for resample_harness.bad_calls with the map fmap; the remap's own rows: a map that is the output buffer
    (so the rows are a function of its address) or is not aligned to its entries, and stage_bytes outside 16..65520."""
    im = fmap.ctypes.data
    make = lambda **kw: mk(pkg, **kw)
    good = (C.byref(mk(pkg)), im)

    def rows(out):
        own = [(8, 8, 3, (good[0], m)) for m in (out, im + 1, im + 2)]
        own += [(8, 8, 3, (C.byref(mk(pkg, stage=st)), im)) for st in (8, 15, 65521, -16)]
        return size_rows(make, (im,)) + sampler_rows(make, (im,)) + own
    return good, rows


def test_cpu_run_refuses_invalid_arguments(pkg, L):
    fmap = identity_map(16, 16)
    a, b = check_cpu_run_refuses(REMAP, pkg, L, *bad_rows(pkg, fmap))
    for stage in (16, 4096, STAGE_MAX):
        assert L.mi_blur_cpu_run_remap(a.ctypes.data, b.ctypes.data, 8, 8, 3, 1, C.byref(mk(pkg, stage=stage)), fmap.ctypes.data, 1) == pkg.OK


def test_enqueue_invalid_comes_before_no_device(pkg, L):
    """Every argument is checked before a device is asked for; without a GPU a good call is ERR_NO_DEVICE (with one, the
    null stream of an empty batch is MI_BLUR_OK)."""
    check_enqueue_invalid_before_no_device(REMAP, pkg, L, *bad_rows(pkg, identity_map(16, 16)))


def test_ctx_set_refuses_invalid_arguments(pkg, L):
    """A null context, struct or map is ERR_INVALID whatever the state, an invalid struct ERR_INVALID before the first
    submit, anything ERR_STATE after it; a refused set leaves the filter in place."""
    fmap = identity_map(16, 16)
    bad = [dict(wo=0), dict(ho=0), dict(wo=MAX_DIM + 1, ho=1), dict(wo=1, ho=MAX_DIM + 1), dict(mode=2), dict(border=2), dict(fill=256), dict(fill=-1), dict(stage=8),
           dict(stage=65521), dict(wo=MAX_DIM, ho=MAX_DIM)]
    check_ctx_set_refuses(REMAP, pkg, L, (C.byref(mk(pkg)), fmap.ctypes.data), [(C.byref(mk(pkg, **kw)), fmap.ctypes.data) for kw in bad])


def test_a_failed_setter_keeps_the_previous_remap_working(pkg, L):
    img = np.random.default_rng(21).integers(0, 256, size=(2, 20, 24, 3), dtype=np.uint8)
    n, h, w, c = img.shape
    rng = np.random.default_rng(22)
    first = wild(rng, w, h, 30, 11)
    with pkg.Context(pkg.DEVICE_CPU, w, h, c, 1, max_batch=n) as ctx:
        ctx.set_remap(make_remap(pkg, 30, 11, BILINEAR, CLAMP), first)
        other = wild(rng, w, h, 40, 31)
        assert L.mi_blur_ctx_set_remap(ctx.h, C.byref(make_remap(pkg, 40, 31, 7)), other.ctypes.data) == pkg.ERR_INVALID
        assert L.mi_blur_ctx_set_remap(ctx.h, C.byref(make_remap(pkg, 40, 31)), None) == pkg.ERR_INVALID
        assert L.mi_blur_ctx_set_warp(ctx.h, C.byref(wr.make_warp(pkg, wr.identity(), 0, 5))) == pkg.ERR_INVALID
        want = ref_remap(img, first, BILINEAR, CLAMP)
        out = np.full(want.size + 64, 0xA5, np.uint8)
        ctx.submit(img.ctypes.data, out.ctypes.data, n)
        ctx.sync()
        assert np.array_equal(out[:want.size].reshape(want.shape), want) and (out[want.size:] == 0xA5).all()


@pytest.mark.parametrize("target", [(42, 37), (63, 74), (25, 22)], ids=lambda t: "x".join(map(str, t)))
def test_cpu_context(pkg, L, target):
    img = np.random.default_rng(23).integers(0, 256, size=(5, 37, 42, 3), dtype=np.uint8)
    n, h, w, c = img.shape
    wo, ho = target
    fmap = build_map("barrel", w, h, wo, ho)
    for mode in MODES:
        for border in BORDERS:
            check_cpu_context(REMAP, pkg, L, img, (fmap, mode, border, 33, 0))


def test_setters_replace_each_other(pkg, L):
    img = np.random.default_rng(29).integers(0, 256, size=(2, 20, 24, 3), dtype=np.uint8)
    n, h, w, c = img.shape
    m = wr.rotation_m(w, h, -40.0)
    rng = np.random.default_rng(30)
    map_a, map_b = wild(rng, w, h, 40, 31), wild(rng, w, h, 17, 9)

    remap_a = lambda ctx: ctx.set_remap(make_remap(pkg, 40, 31, BILINEAR, CLAMP), map_a)
    remap_b = lambda ctx: ctx.set_remap(make_remap(pkg, 17, 9, NEAREST, CONSTANT, 5), map_b)
    warp = lambda ctx: ctx.set_warp(wr.make_warp(pkg, m, 40, 31, BILINEAR, CLAMP))
    median = lambda ctx: ctx.set_median(1)
    ra, rb = ref_remap(img, map_a, BILINEAR, CLAMP), ref_remap(img, map_b, NEAREST, CONSTANT, 5)
    rot, med = wr.ref_warp(img, m, 40, 31, BILINEAR, CLAMP), cpu_run_same_size(MEDIAN, pkg, L, img, 1, 1)
    check_setters_replace_each_other(pkg, L, img, [([remap_a, warp], rot), ([warp, remap_a], ra), ([remap_a, median], med), ([median, remap_b], rb),      # the last one wins
                                                   ([remap_a, remap_b], rb), ([remap_b, remap_a, remap_b, remap_a], ra)])   # a remap replaces a remap: the first map is freed


def test_numpy_functions_on_the_cpu_device(pkg, L):
    rng = np.random.default_rng(31)
    stack = rng.integers(0, 256, size=(4, 45, 71, 3), dtype=np.uint8)
    xs, ys = (rng.uniform(-4, 80, size=(33, 50)) for _ in range(2))
    fmap = quantise(xs.astype(np.float32), ys.astype(np.float32))
    for img in (stack, stack[0], np.ascontiguousarray(stack[0, :, :, 0])):
        as4 = img if img.ndim == 4 else img[None] if img.ndim == 3 else img[None, :, :, None]
        shape = lambda want: want.reshape(want.shape if img.ndim == 4 else want.shape[1:] if img.ndim == 3 else want.shape[1:3])
        for mode, mo in (("bilinear", BILINEAR), ("nearest", NEAREST)):
            for border, bo in (("constant", CONSTANT), ("clamp", CLAMP)):
                want = shape(ref_remap(as4, fmap, mo, bo, 9))
                got = pkg.remap(img, xs, ys, mode, border, 9, device=pkg.DEVICE_CPU, batch=3)         # a float pair
                assert got.shape == want.shape and got.ndim == img.ndim and np.array_equal(got, want), (img.ndim, mode, border)
                assert np.array_equal(pkg.remap(img, fmap, None, mode, border, 9, device=pkg.DEVICE_CPU), want)   # a fixed-point map
    K = barrel_K(71, 45)
    assert np.array_equal(pkg.undistort(stack, K, BARREL_DIST, device=pkg.DEVICE_CPU), ref_remap(stack, pkg.undistort_map(K, BARREL_DIST, (71, 45)), BILINEAR, CONSTANT, 0))
    got = pkg.undistort(stack[0], K, BARREL_DIST[:2], K, (50, 60), "nearest", "clamp", device=pkg.DEVICE_CPU)
    assert np.array_equal(got, ref_remap(stack[:1], pkg.undistort_map(K, list(BARREL_DIST[:2]) + [0, 0, 0], (50, 60)), NEAREST, CLAMP)[0])
    empty = pkg.remap(np.zeros((0, 45, 71, 3), np.uint8), fmap, device=pkg.DEVICE_CPU)
    assert empty.shape == (0, 33, 50, 3) and empty.dtype == np.uint8
    for bad in (dict(mode="cubic"), dict(border="reflect"), dict(fill=256)):
        with pytest.raises(ValueError):
            pkg.remap(stack, fmap, device=pkg.DEVICE_CPU, **bad)
    with pytest.raises(ValueError):
        pkg.remap(stack, fmap.astype(np.int64), device=pkg.DEVICE_CPU)
    with pytest.raises(ValueError):
        pkg.remap(stack, xs, ys[:5], device=pkg.DEVICE_CPU)
    with pytest.raises(pkg.MiBlurError):
        pkg.remap(stack, np.full((4, 4), np.nan), np.zeros((4, 4)), device=pkg.DEVICE_CPU)
    with pytest.raises(pkg.MiBlurError):
        pkg.remap(stack, fmap, stage_bytes=8, device=pkg.DEVICE_CPU)


# ---------------------------------------------------------------- hosts
def host_undistort_map(pkg, w, h, k):
    return pkg.undistort_map(barrel_K(w, h), list(k) + [0.0] * (5 - len(k)), (w, h))


def test_hosts_refuse_undistort_with_other_filters(pkg, tmp_path):
    pkg.build_native()
    het, split = os.path.join(pkg.APPS, "heterogeneous_blur"), os.path.join(pkg.APPS, "split_image_blur")
    base = ["cpu", "0", "35", "--size", "32x24", "--images", "4", "--undistort", "-0.2"]
    for extra in (["--sigma", "1.0"], ["--median", "3"], ["--erode", "3"], ["--bilateral", "5"], ["--conv", "sobel"], ["--pyr-down"], ["--ksize", "5"],
                  ["--resize", "64x48"], ["--rotate", "30"], ["--perspective", "0,0,31,0,31,23,0,23"], ["--resident"], ["--frames", str(tmp_path)]):
        r = subprocess.run([het, *base, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "excludes" in r.stdout and "--undistort" in r.stdout, (extra, r.stdout[-500:])
    for bad in (["--undistort", "abc"], ["--undistort", "0.1,0.2,0.3"], ["--undistort", "0.1,0.2,0.3,0.4,0.5,0.6"], ["--undistort", "0.1x"]):
        r = subprocess.run([het, "cpu", "0", "35", "--size", "32x24", "--images", "4", *bad], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Error: --undistort k1[,k2[,p1,p2[,k3]]]" in r.stdout, bad
    r = subprocess.run([split, "0.5", "35", "--size", "32x24", "--images", "4", "--undistort", "-0.2"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--undistort" in r.stdout and "bands are not supported" in r.stdout


def test_host_undistorts_on_the_cpu_device(pkg, tmp_path):
    from resample_harness import read_ppm, write_ppm
    pkg.build_native()
    het = os.path.join(pkg.APPS, "heterogeneous_blur")
    img = np.random.default_rng(19).integers(0, 256, size=(48, 64, 3), dtype=np.uint8)
    src = tmp_path / "in.ppm"
    write_ppm(src, img)
    for arg, k, flags, mode, border, fill, name in (("-0.2", [-0.2], [], BILINEAR, CLAMP, 0, "bilinear"),
                                                     ("-0.2,0.05,0.001,-0.002,0.01", BARREL_DIST, ["--nearest", "--border-fill", "77"], NEAREST, CONSTANT, 77, "nearest")):
        dst = tmp_path / f"{name}.ppm"
        r = subprocess.run([het, "cpu", "0", "35", "--image", str(src), "--images", "4", "--undistort", arg, *flags, "--save", str(dst)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert f"Blur kernel: {name} remap, undistort k1=-0.2, 64x48 -> 64x48" in r.stdout
        assert np.array_equal(read_ppm(dst), ref_remap(img[None], host_undistort_map(pkg, 64, 48, k), mode, border, fill)[0]), name


# ---------------------------------------------------------------- the kernels, without a GPU
def test_tiled_kernels_use_no_scratch(pkg, tmp_path):
    """Compiles remap_kernels.hip to gfx950 assembly (no GPU needed): the map entries stay in registers, so no tiled
    instantiation may spill or index registers at run time; all LDS is dynamic."""
    no_scratch(pkg, tmp_path, "remap_kernels.hip", "blur_remap_tiled_kernel", 4, dynamic_lds_only=True)     # 1-4 channels


@needs_gxx
def test_cpu_remap_and_the_tile_walk_clean_under_asan_ubsan(pkg, tmp_path):
    """tests/san_remap.cpp: the CPU device in exact-size heap buffers on random, extreme and the GPU tests' maps, and every
    LDS offset a staged tile of the mixed, rot30 and wild maps would read, against stage_bytes + WARP_LDS_SLACK."""
    run_sanitized(pkg, tmp_path, ("san_remap.cpp", "cpu_device.cpp"), ["remap cases clean", "taps inside their LDS"])
