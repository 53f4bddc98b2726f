"""The image resize (mi_blur_resize_coord, mi_blur_cpu_run_resize, mi_blur_enqueue_resize's argument checks,
mi_blur_ctx_set_resize, resize() / resize_coord()), CPU only: against the numpy restatement of the header's definition
(resize_ref.py), independent of the product.  All comparisons are exact unless stated."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from filter_harness import MEDIAN, cpu_run as cpu_run_same_size
from resample_harness import (RESIZE, check_cpu_context, check_cpu_run_refuses, check_ctx_set_refuses, check_enqueue_invalid_before_no_device,
                              check_setters_replace_each_other, cpu_run, needs_gxx, no_scratch, run_sanitized, size_rows)
from resize_ref import BILINEAR, MAX_DIM, NEAREST, float_bilinear, ref_axis, ref_resize
from sep_down_ref import ref_sep_down
from sep_ref import rand_taps

SHAPES = [(3, 33, 40, 3), (1, 1, 1, 3), (2, 9, 5, 1), (1, 17, 16, 4), (1, 50, 7, 5), (1, 64, 96, 2)]
MODES = (BILINEAR, NEAREST)


def targets(h, w):
    """(Wo, Ho): same size, 2x, (2W+1) x (3H-1) capped at 1, 1 x 1, about 0.6x, one axis up with the other down."""
    return [(w, h), (2 * w, 2 * h), (2 * w + 1, max(3 * h - 1, 1)), (1, 1), (max(1, round(0.6 * w)), max(1, round(0.6 * h))),
            (w + (w + 1) // 2, max(1, h // 2))]


def test_coord_equals_the_restatement(pkg, L):
    a, b, f = C.c_int(), C.c_int(), C.c_int()
    for mode in MODES:
        for n_in in range(1, 41):
            for n_out in range(1, 41):
                ra, rb, rf = ref_axis(n_in, n_out, mode)
                got = []
                for X in range(n_out):
                    assert L.mi_blur_resize_coord(n_in, n_out, mode, X, C.byref(a), C.byref(b), C.byref(f)) == pkg.OK
                    got.append((a.value, b.value, f.value))
                g = np.array(got, dtype=np.int64)
                assert np.array_equal(g[:, 0], ra) and np.array_equal(g[:, 1], rb) and np.array_equal(g[:, 2], rf), (mode, n_in, n_out)
                assert (g[:, 0] <= g[:, 1]).all() and (g[:, 1] <= g[:, 0] + 1).all() and (g[:, 0] >= 0).all() and (g[:, 1] < n_in).all()
                assert (g[:, 2] >= 0).all() and (g[:, 2] <= 2048).all() and (np.diff(g[:, 0]) >= 0).all(), (mode, n_in, n_out)
                if mode == NEAREST:
                    assert np.array_equal(g[:, 0], g[:, 1]) and not g[:, 2].any()
                if n_in == n_out:                                        # the identity
                    assert np.array_equal(g[:, 0], np.arange(n_in)) and not g[:, 2].any()
    assert pkg.resize_coord(7, 20, 0) == tuple(int(v[0]) for v in ref_axis(7, 20))
    assert pkg.resize_coord(7, 20, 19, "nearest") == (6, 6, 0)
    # the largest sizes stay inside 32 bits
    for n_in, n_out in ((MAX_DIM, MAX_DIM), (MAX_DIM, 1), (1, MAX_DIM), (MAX_DIM, MAX_DIM - 1), (MAX_DIM - 1, MAX_DIM), (3, MAX_DIM)):
        for mode in MODES:
            ra, rb, rf = ref_axis(n_in, n_out, mode)
            for X in sorted({0, 1, n_out // 2, n_out - 2, n_out - 1} & set(range(n_out))):
                assert pkg.resize_coord(n_in, n_out, X, mode) == (ra[X], rb[X], rf[X]), (n_in, n_out, mode, X)
    for bad in ((0, 4, 1, 0), (4, 0, 1, 0), (MAX_DIM + 1, 4, 1, 0), (4, MAX_DIM + 1, 1, 0), (4, 4, 2, 0), (4, 4, -1, 0), (4, 4, 1, 4), (4, 4, 1, -1)):
        assert L.mi_blur_resize_coord(*bad, C.byref(a), C.byref(b), C.byref(f)) == pkg.ERR_INVALID, bad
    assert L.mi_blur_resize_coord(4, 4, 1, 0, None, C.byref(b), C.byref(f)) == pkg.ERR_INVALID


def test_properties_of_the_definition(pkg, L):
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(2, 13, 17, 3), dtype=np.uint8)
    for mode in MODES:
        assert np.array_equal(cpu_run(RESIZE, pkg, L, img, (17, 13, mode), 2), img)                   # same size: the identity
        for v in (0, 200, 255):
            flat = np.full((1, 9, 11, 2), v, np.uint8)
            for wo, ho in ((11, 9), (30, 31), (5, 4), (1, 1), (64, 3)):
                assert (cpu_run(RESIZE, pkg, L, flat, (wo, ho, mode), 1) == v).all(), (mode, v, wo, ho)
                assert (ref_resize(flat, wo, ho, mode) == v).all()
    for k in (2, 3):
        want = np.repeat(np.repeat(img, k, axis=1), k, axis=2)
        assert np.array_equal(cpu_run(RESIZE, pkg, L, img, (17 * k, 13 * k, NEAREST), 2), want), k


@pytest.mark.parametrize("case", [(33, 48, 67, 131), (40, 64, 25, 37), (31, 17, 93, 51), (7, 5, 64, 64)], ids=lambda c: "x".join(map(str, c)))
def test_bilinear_is_within_one_of_float_bilinear(pkg, L, case):
    """Against float64 half-pixel bilinear rounded half up, on a 0/255 checkerboard with noise: at most 1 apart (the
    header's bound: the fixed-point value is less than 0.63 from the real one)."""
    h, w, wo, ho = case
    rng = np.random.default_rng(h * w)
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((yy + xx) & 1) * 255).astype(np.int64)[None, :, :, None] + rng.integers(-20, 21, size=(2, h, w, 3))
    img = np.clip(board, 0, 255).astype(np.uint8)
    real = float_bilinear(img, wo, ho)
    exact = np.floor(real + 0.5).astype(np.int64)
    restated = ref_resize(img, wo, ho)
    got = cpu_run(RESIZE, pkg, L, img, (wo, ho, BILINEAR), 2)
    assert np.array_equal(got, restated)
    assert np.abs(restated.astype(np.int64) - exact).max() <= 1
    assert np.abs(restated.astype(np.float64) - real).max() < 0.5 + 2 * 255 / 4096


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cpu_run_matches_the_restatement(pkg, L, shape):
    rng = np.random.default_rng(sum(shape))
    img = rng.integers(0, 256, size=shape, dtype=np.uint8)
    n, h, w, c = shape
    for wo, ho in targets(h, w):
        for mode in MODES:
            want = ref_resize(img, wo, ho, mode)
            assert want.shape == (n, ho, wo, c)
            for nt in (1, 4):
                assert np.array_equal(cpu_run(RESIZE, pkg, L, img, (wo, ho, mode), nt), want), (shape, wo, ho, mode, nt)


def bad_rows(pkg):
    """(good, rows) for resample_harness.bad_calls: resize has no rows of its own."""
    mk = lambda wo=16, ho=16, mode=BILINEAR: pkg.Resize(wo, ho, mode)
    return (C.byref(mk()),), size_rows(mk)


def test_cpu_run_refuses_invalid_arguments(pkg, L):
    check_cpu_run_refuses(RESIZE, pkg, L, *bad_rows(pkg))


def test_enqueue_invalid_comes_before_no_device(pkg, L):
    """Every argument is checked before a device is asked for; without a GPU a good call is ERR_NO_DEVICE (with one, the
    null stream of an empty batch is MI_BLUR_OK)."""
    check_enqueue_invalid_before_no_device(RESIZE, pkg, L, *bad_rows(pkg))


def test_ctx_set_refuses_invalid_arguments(pkg, L):
    bad = [(C.byref(pkg.Resize(*r)),) for r in [(0, 16, 1), (16, 0, 1), (MAX_DIM + 1, 1, 1), (1, MAX_DIM + 1, 1), (16, 16, 2), (MAX_DIM, MAX_DIM, 1)]]
    check_ctx_set_refuses(RESIZE, pkg, L, (C.byref(pkg.Resize(16, 16, 1)),), bad)


@pytest.mark.parametrize("target", [(84, 70), (63, 74), (25, 22), (60, 20)], ids=lambda t: "x".join(map(str, t)))
def test_cpu_context(pkg, L, target):
    rng = np.random.default_rng(23)
    img = rng.integers(0, 256, size=(5, 37, 42, 3), dtype=np.uint8)
    wo, ho = target
    for mode in MODES:
        check_cpu_context(RESIZE, pkg, L, img, (wo, ho, mode))


def test_setters_replace_each_other(pkg, L):
    rng = np.random.default_rng(29)
    img = rng.integers(0, 256, size=(2, 20, 24, 3), dtype=np.uint8)
    k = pkg.SepKernel.from_taps(rand_taps(rng, 2), rand_taps(rng, 1))

    resize = lambda ctx: ctx.set_resize(40, 31)
    median = lambda ctx: ctx.set_median(1)
    down = lambda ctx: ctx.set_sep_down(k, 2, 2, 1, 0)
    big, med, dec = ref_resize(img, 40, 31), cpu_run_same_size(MEDIAN, pkg, L, img, 1, 1), ref_sep_down(img, *k.taps(), 2, 2, 1, 0)
    check_setters_replace_each_other(pkg, L, img, [([resize, median], med), ([median, resize], big), ([resize, down], dec), ([down, resize], big)])   # the last one wins


def test_numpy_function_on_the_cpu_device(pkg, L):
    rng = np.random.default_rng(31)
    stack = rng.integers(0, 256, size=(4, 45, 71, 3), dtype=np.uint8)
    for img in (stack, stack[0], np.ascontiguousarray(stack[0, :, :, 0])):
        as4 = img if img.ndim == 4 else img[None] if img.ndim == 3 else img[None, :, :, None]
        shape = lambda want: want.reshape(want.shape if img.ndim == 4 else want.shape[1:] if img.ndim == 3 else want.shape[1:3])
        for size in ((142, 90), (100, 33), (71, 45)):
            for mode, m in (("bilinear", BILINEAR), ("nearest", NEAREST)):
                got = pkg.resize(img, size, mode, device=pkg.DEVICE_CPU, batch=3)
                want = shape(ref_resize(as4, *size, m))
                assert got.shape == want.shape and got.ndim == img.ndim and np.array_equal(got, want), (img.ndim, size, mode)
    assert np.array_equal(pkg.resize(stack, (142, 90), device=pkg.DEVICE_CPU), ref_resize(stack, 142, 90))      # bilinear by default
    empty = pkg.resize(np.zeros((0, 45, 71, 3), np.uint8), (10, 20), device=pkg.DEVICE_CPU)
    assert empty.shape == (0, 20, 10, 3) and empty.dtype == np.uint8
    with pytest.raises(ValueError):
        pkg.resize(stack, (10, 20), "cubic", device=pkg.DEVICE_CPU)
    with pytest.raises(ValueError):
        pkg.resize(stack, (0, 20), device=pkg.DEVICE_CPU)
    with pytest.raises(ValueError):
        pkg.resize(stack.astype(np.float32), (10, 20), device=pkg.DEVICE_CPU)
    with pytest.raises(pkg.MiBlurError):
        pkg.resize(stack, (MAX_DIM + 1, 20), device=pkg.DEVICE_CPU)


def test_hosts_refuse_resize_with_other_filters(pkg, tmp_path):
    """The command lines are refused while the flags are parsed, before any device is asked for."""
    pkg.build_native()
    het, split = os.path.join(pkg.APPS, "heterogeneous_blur"), os.path.join(pkg.APPS, "split_image_blur")
    base = ["cpu", "0", "35", "--size", "32x24", "--images", "4", "--resize", "64x48"]
    for extra in (["--sigma", "1.0"], ["--median", "3"], ["--erode", "3"], ["--dilate", "3"], ["--morph-gradient", "3"], ["--bilateral", "5"],
                  ["--conv", "sobel"], ["--pyr-down"], ["--ksize", "5"], ["--resident"], ["--frames", str(tmp_path)]):
        r = subprocess.run([het, *base, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Error: --resize excludes" in r.stdout, extra
    r = subprocess.run([het, "cpu", "0", "35", "--size", "32x24", "--images", "4", "--nearest"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Error: --nearest needs --resize" in r.stdout
    for bad in ("64", "64x", "0x48", "64x48x3", "40000x10"):
        r = subprocess.run([het, "cpu", "0", "35", "--size", "32x24", "--images", "4", "--resize", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Error: --resize WxH" in r.stdout, bad
    r = subprocess.run([split, "0.5", "35", "--size", "32x24", "--images", "4", "--resize", "64x48"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--resize" in r.stdout and "bands are not supported" in r.stdout


def test_tiled_kernels_use_no_scratch(pkg, tmp_path):
    """Compiles resize_kernels.hip to gfx950 assembly (no GPU needed): the gather of the horizontal pass reads LDS at
    run-time addresses, but no tiled instantiation may spill or index registers at run time."""
    no_scratch(pkg, tmp_path, "resize_kernels.hip", "blur_resize_tiled_kernel", 4)       # 1-4 channels


@needs_gxx
def test_cpu_resize_clean_under_asan_ubsan(pkg, tmp_path):
    run_sanitized(pkg, tmp_path, ("san_resize.cpp", "cpu_device.cpp"), ["400 random resize cases clean"])
