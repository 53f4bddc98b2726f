"""The area resize (mi_blur_area_coord, mi_blur_cpu_run_area, mi_blur_enqueue_area's argument checks, mi_blur_ctx_set_area,
area_resize() / area_coord()), CPU only: against the numpy restatement of the header's definition (area_ref.py),
independent of the product.  All comparisons are exact unless stated."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from area_ref import AREA, MAX_DIM, MAX_RATIO, float_area, ref_area, ref_axis, ref_weights
from filter_harness import MEDIAN, cpu_run as cpu_run_same_size
from resample_harness import (check_cpu_context, check_cpu_run_refuses, check_ctx_set_refuses, check_enqueue_invalid_before_no_device,
                              check_setters_replace_each_other, cpu_run, needs_gxx, no_scratch, run_sanitized)
from resize_ref import ref_resize
from sep_down_ref import ref_sep_down
from sep_ref import rand_taps

# equal sizes, / 2, / 3, / 64, coprime pairs, enlargements, one output, one input, the largest axis
PAIRS = [(1, 1), (7, 7), (40, 40), (16, 8), (15, 5), (128, 2), (64, 1), (7, 5), (100, 37), (64, 63), (1000, 281), (5, 7), (3, 12), (1, 9), (37, 100),
         (9, 1), (1, 1), (MAX_DIM, 512), (MAX_DIM, MAX_DIM), (MAX_DIM, MAX_DIM - 1), (MAX_DIM - 1, MAX_DIM), (1, MAX_DIM), (MAX_DIM, 1)]
SHAPES = [(3, 33, 40, 3), (1, 1, 1, 3), (2, 9, 5, 1), (1, 17, 16, 4), (1, 50, 7, 5), (1, 64, 96, 2)]


def targets(h, w):
    """(Wo, Ho): same size, / 2 (rounded up), about 0.6x, the smallest valid output (1 x 1 up to 64 x 64), coprime reductions,
    2x, one axis up with the other down."""
    return [(w, h), (-(-w // 2), -(-h // 2)), (max(1, round(0.6 * w)), max(1, round(0.6 * h))), (-(-w // MAX_RATIO), -(-h // MAX_RATIO)), (max(1, w - 1), max(1, h - 3)),
            (2 * w, 2 * h), (w + (w + 1) // 2, max(1, h // 2)), (max(1, w // 3), 2 * h + 1)]


def test_coord_equals_the_restatement(pkg, L):
    out = [C.c_int() for _ in range(4)]
    refs = [C.byref(v) for v in out]
    for n_in, n_out in PAIRS:
        i_lo, i_hi, w_lo, w_hi = ref_axis(n_in, n_out)
        xs = range(n_out) if n_out <= 1024 else sorted({0, 1, 2, n_out // 3, n_out // 2, n_out - 3, n_out - 2, n_out - 1})
        got = []
        for X in xs:
            assert L.mi_blur_area_coord(n_in, n_out, X, *refs) == pkg.OK
            got.append(tuple(v.value for v in out))
        g = np.array(got, dtype=np.int64)
        xs = np.array(list(xs))
        assert np.array_equal(g, np.stack([i_lo[xs], i_hi[xs], w_lo[xs], w_hi[xs]], axis=1)), (n_in, n_out)
        taps = g[:, 1] - g[:, 0] + 1
        assert (g[:, 0] >= 0).all() and (g[:, 1] < n_in).all() and (taps >= 1).all() and (taps <= -(-n_in // n_out) + 1).all()
        assert (g[:, 2] > 0).all() and ((g[:, 3] > 0) == (taps > 1)).all() and (g[taps == 1, 2] == n_in).all()
        assert (g[:, 2] + g[:, 3] + np.maximum(taps - 2, 0) * n_out == n_in).all(), (n_in, n_out)      # the weights of an output sum to n_in
        if len(xs) == n_out:
            assert (np.diff(g[:, 0]) >= 0).all() and (np.diff(g[:, 1]) >= 0).all() and (g[1:, 0] >= g[:-1, 1]).all()   # monotone, and sharing at most a boundary tap
            assert g[0, 0] == 0 and g[-1, 1] == n_in - 1
        if n_in == n_out:                                                # the identity
            assert np.array_equal(g[:, 0], xs) and (taps == 1).all()
    for n_in, n_out in [p for p in PAIRS if p[0] * p[1] <= 1 << 16]:     # the form of mi_blur_area_coord against the matrix of the header's w(X, i)
        m = ref_weights(n_in, n_out)
        i_lo, i_hi, w_lo, w_hi = ref_axis(n_in, n_out)
        assert (m.sum(axis=1) == n_in).all() and (m.sum(axis=0) == n_out).all()
        for X in range(n_out):
            row = np.zeros(n_in, np.int64)
            row[i_lo[X]:i_hi[X] + 1] = n_out
            row[i_lo[X]] = w_lo[X]
            if i_hi[X] > i_lo[X]:
                row[i_hi[X]] = w_hi[X]
            assert np.array_equal(row, m[X]), (n_in, n_out, X)
    assert pkg.area_coord(7, 5, 0) == (0, 1, 5, 2) and pkg.area_coord(7, 5, 4) == (5, 6, 2, 5) and pkg.area_coord(5, 5, 3) == (3, 3, 5, 0)
    for bad in ((0, 4, 0), (4, 0, 0), (MAX_DIM + 1, 4, 0), (4, MAX_DIM + 1, 0), (4, 4, 4), (4, 4, -1)):
        assert L.mi_blur_area_coord(*bad, *refs) == pkg.ERR_INVALID, bad
    for j in range(4):
        assert L.mi_blur_area_coord(4, 4, 0, *refs[:j], None, *refs[j + 1:]) == pkg.ERR_INVALID


@pytest.mark.parametrize("nt", [1, 3])
def test_properties_of_the_definition(pkg, L, nt):
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(2, 12, 18, 3), dtype=np.uint8)
    run = lambda a, wo, ho: cpu_run(AREA, pkg, L, a, (wo, ho), nt)
    assert np.array_equal(run(img, 18, 12), img)                         # same size: the identity
    for v in (0, 1, 200, 255):                                           # a constant image stays constant
        flat = np.full((1, 9, 11, 2), v, np.uint8)
        for wo, ho in ((11, 9), (30, 31), (5, 4), (1, 1), (64, 3), (7, 9)):
            assert (run(flat, wo, ho) == v).all(), (v, wo, ho)
            assert (ref_area(flat, wo, ho) == v).all()
    for k in (2, 3, 6):                                                  # an integer reduction: the mean of each k x k block, rounded half up
        blocks = img.astype(np.int64).reshape(2, 12 // k, k, 18 // k, k, 3).sum(axis=(2, 4))
        want = (2 * blocks + k * k) // (2 * k * k)
        got = run(img, 18 // k, 12 // k)
        assert np.array_equal(got, want), k
        if k == 2:                                                       # never below the truncating preset, at most 1 above
            assert np.array_equal(want, (blocks + 2) >> 2)
            trunc = pkg.area_down(img, 2, device=pkg.DEVICE_CPU).astype(np.int64)
            assert ((got - trunc) >= 0).all() and ((got - trunc) <= 1).all() and (got != trunc).any()
    for k in (2, 3):                                                     # an integer enlargement replicates pixels
        assert np.array_equal(run(img, 18 * k, 12 * k), np.repeat(np.repeat(img, k, axis=1), k, axis=2)), k
    for wo, ho in ((7, 5), (13, 11), (25, 7), (5, 17), (1, 1)):          # within 0.5 of the real-valued box average
        got = run(img, wo, ho)
        assert np.array_equal(got, ref_area(img, wo, ho))
        assert np.abs(got.astype(np.float64) - float_area(img, wo, ho)).max() <= 0.5 + 1e-9, (wo, ho)
    # the order of the two passes cannot change S: x then y, y then x, both with the one rounding at the end
    v = img.astype(np.int64)
    wx, wy = ref_weights(18, 7), ref_weights(12, 5)
    assert np.array_equal(np.einsum("yj,njxc->nyxc", wy, np.einsum("xi,njic->njxc", wx, v)), np.einsum("xi,nyic->nyxc", wx, np.einsum("yj,njic->nyic", wy, v)))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cpu_run_matches_the_restatement(pkg, L, shape):
    rng = np.random.default_rng(sum(shape))
    img = rng.integers(0, 256, size=shape, dtype=np.uint8)
    n, h, w, c = shape
    for wo, ho in targets(h, w):
        want = ref_area(img, wo, ho)
        assert want.shape == (n, ho, wo, c)
        for nt in (1, 4):
            assert np.array_equal(cpu_run(AREA, pkg, L, img, (wo, ho), nt), want), (shape, wo, ho, nt)


def test_totals_are_64_bit(pkg, L):
    """8192 x 4096 x 1 of 255 -> 128 x 64: S = 255 * 2^25 per output, the numerator 2 S + D over 2^34.  A 32-bit total
    anywhere gives something other than 255."""
    img = np.full((1, 4096, 8192, 1), 255, np.uint8)
    assert (cpu_run(AREA, pkg, L, img, (128, 64), 4) == 255).all()
    img[0, ::2] = 0                                                      # every other row black: 127.5 rounds half up
    assert (cpu_run(AREA, pkg, L, img, (128, 64), 4) == 128).all()


def bad_rows(pkg):
    """(good, rows) for resample_harness.bad_calls, made on an 8 x 8 x 3 input: the sizes and byte limits of the resize (no
    mode here, so not size_rows()), and this family's own: a reduction by more than MAX_RATIO on either axis."""
    row = lambda w, h, c, wo=16, ho=16: (w, h, c, (C.byref(pkg.Area(wo, ho)),))
    rows = [row(w, h, c) for w, h, c in [(0, 8, 3), (8, 0, 3), (8, 8, 0), (-1, 8, 3), (MAX_DIM + 1, 1, 1), (1, MAX_DIM + 1, 1)]]
    rows += [row(8, 8, 3, **kw) for kw in [dict(wo=0), dict(ho=0), dict(wo=-3), dict(ho=-1), dict(wo=MAX_DIM + 1, ho=1), dict(wo=1, ho=MAX_DIM + 1)]]
    rows.append(row(8, 8, 3, wo=MAX_DIM, ho=MAX_DIM))                    # the output image: 3 GiB, over the per-image limit
    rows.append(row(8, 8, 40000, wo=MAX_DIM, ho=1))                      # the output row: over INT_MAX / 2
    rows += [row(65, 8, 3, wo=1), row(8, 65, 3, ho=1), row(2 * MAX_RATIO + 1, 1, 1, wo=2, ho=1), row(1, 3 * MAX_RATIO + 1, 1, wo=1, ho=3)]
    return (C.byref(pkg.Area(16, 16)),), rows


def test_cpu_run_refuses_invalid_arguments(pkg, L):
    check_cpu_run_refuses(AREA, pkg, L, *bad_rows(pkg))
    # a ratio of exactly MAX_RATIO is taken on either axis, one more is not
    for shape, spec, ok in [((1, 2, 64, 1), (1, 2), True), ((1, 2, 65, 1), (1, 2), False), ((1, 128, 3, 2), (3, 2), True), ((1, 129, 3, 2), (3, 2), False),
                            ((1, 128, 128, 1), (2, 2), True), ((1, 128, 129, 1), (2, 2), False)]:
        img = np.random.default_rng(5).integers(0, 256, size=shape, dtype=np.uint8)
        out = np.zeros((shape[0], spec[1], spec[0], shape[3]), np.uint8)
        rc = AREA.cpu_run(L, img.ctypes.data, out.ctypes.data, shape[2], shape[1], shape[3], 1, AREA.host_args(pkg, spec), 1)
        assert rc == (pkg.OK if ok else pkg.ERR_INVALID), (shape, spec)
        if ok:
            assert np.array_equal(out, ref_area(img, *spec))


def test_enqueue_invalid_comes_before_no_device(pkg, L):
    """Every argument is checked before a device is asked for; without a GPU a good call is ERR_NO_DEVICE (with one, the
    null stream of an empty batch is MI_BLUR_OK)."""
    check_enqueue_invalid_before_no_device(AREA, pkg, L, *bad_rows(pkg))


def test_ctx_set_refuses_invalid_arguments(pkg, L):
    bad = [(C.byref(pkg.Area(*r)),) for r in [(0, 16), (16, 0), (MAX_DIM + 1, 1), (1, MAX_DIM + 1), (-1, 4), (MAX_DIM, MAX_DIM)]]
    check_ctx_set_refuses(AREA, pkg, L, (C.byref(pkg.Area(16, 16)),), bad)
    with pkg.Context(pkg.DEVICE_CPU, 130, 65, 1, 1, max_batch=1) as ctx:                 # the ratio against the context's own size
        assert L.mi_blur_ctx_set_area(ctx.h, C.byref(pkg.Area(2, 2))) == pkg.ERR_INVALID
        assert L.mi_blur_ctx_set_area(ctx.h, C.byref(pkg.Area(3, 1))) == pkg.ERR_INVALID
        assert L.mi_blur_ctx_set_area(ctx.h, C.byref(pkg.Area(3, 2))) == pkg.OK


@pytest.mark.parametrize("target", [(21, 18), (16, 9), (42, 37), (60, 20)], ids=lambda t: "x".join(map(str, t)))
def test_cpu_context(pkg, L, target):
    rng = np.random.default_rng(23)
    img = rng.integers(0, 256, size=(5, 37, 42, 3), dtype=np.uint8)
    check_cpu_context(AREA, pkg, L, img, target)


def test_setters_replace_each_other(pkg, L):
    rng = np.random.default_rng(29)
    img = rng.integers(0, 256, size=(2, 20, 24, 3), dtype=np.uint8)
    k = pkg.SepKernel.from_taps(rand_taps(rng, 2), rand_taps(rng, 1))

    area = lambda ctx: ctx.set_area(9, 7)
    resize = lambda ctx: ctx.set_resize(40, 31)
    median = lambda ctx: ctx.set_median(1)
    down = lambda ctx: ctx.set_sep_down(k, 2, 2, 1, 0)
    small, big = ref_area(img, 9, 7), ref_resize(img, 40, 31)
    med, dec = cpu_run_same_size(MEDIAN, pkg, L, img, 1, 1), ref_sep_down(img, *k.taps(), 2, 2, 1, 0)
    check_setters_replace_each_other(pkg, L, img, [([area, resize], big), ([resize, area], small), ([area, median], med), ([median, area], small),
                                                   ([area, down], dec), ([down, area], small)])   # the last one wins


def test_numpy_function_on_the_cpu_device(pkg, L):
    rng = np.random.default_rng(31)
    stack = rng.integers(0, 256, size=(4, 45, 71, 3), dtype=np.uint8)
    for img in (stack, stack[0], np.ascontiguousarray(stack[0, :, :, 0])):
        as4 = img if img.ndim == 4 else img[None] if img.ndim == 3 else img[None, :, :, None]
        shape = lambda want: want.reshape(want.shape if img.ndim == 4 else want.shape[1:] if img.ndim == 3 else want.shape[1:3])
        for size in ((30, 20), (100, 33), (71, 45), (2, 1)):
            got = pkg.area_resize(img, size, device=pkg.DEVICE_CPU, batch=3)
            want = shape(ref_area(as4, *size))
            assert got.shape == want.shape and got.ndim == img.ndim and np.array_equal(got, want), (img.ndim, size)
    empty = pkg.area_resize(np.zeros((0, 45, 71, 3), np.uint8), (10, 20), device=pkg.DEVICE_CPU)
    assert empty.shape == (0, 20, 10, 3) and empty.dtype == np.uint8
    with pytest.raises(ValueError):
        pkg.area_resize(stack, (0, 20), device=pkg.DEVICE_CPU)
    with pytest.raises(ValueError):
        pkg.area_resize(stack.astype(np.float32), (10, 20), device=pkg.DEVICE_CPU)
    with pytest.raises(pkg.MiBlurError):
        pkg.area_resize(stack, (MAX_DIM + 1, 20), device=pkg.DEVICE_CPU)
    with pytest.raises(pkg.MiBlurError):
        pkg.area_resize(stack, (1, 20), device=pkg.DEVICE_CPU)            # 71 -> 1: over MAX_RATIO
    assert pkg.AREA_MAX_RATIO == MAX_RATIO


def test_hosts_area_flag(pkg, tmp_path):
    """--area is refused with --nearest and without --resize while the flags are parsed; with --resize it runs on the CPU
    device and prints the area banner."""
    pkg.build_native()
    het = os.path.join(pkg.APPS, "heterogeneous_blur")
    base = [het, "cpu", "0", "35", "--size", "32x24", "--images", "4"]
    r = subprocess.run([*base, "--resize", "16x12", "--area", "--nearest"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Error: --area excludes --nearest" in r.stdout
    r = subprocess.run([*base, "--area"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Error: --area needs --resize" in r.stdout
    r = subprocess.run([*base, "--resize", "16x12", "--area", "--median", "3"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Error: --resize excludes" in r.stdout
    r = subprocess.run([*base, "--resize", "16x12", "--area"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Blur kernel: area resize, 32x24 -> 16x12" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_tiled_kernels_use_no_scratch(pkg, tmp_path):
    """Compiles area_kernels.hip to gfx950 assembly (no GPU needed): the horizontal pass reads LDS at run-time addresses,
    but no tiled instantiation may spill or index registers at run time, and all their LDS is sized per launch."""
    no_scratch(pkg, tmp_path, "area_kernels.hip", "blur_area_tiled_kernel", 4, dynamic_lds_only=True)       # 1-4 channels


@needs_gxx
def test_area_clean_under_asan_ubsan(pkg, tmp_path):
    run_sanitized(pkg, tmp_path, ("san_area.cpp", "cpu_device.cpp"), ["tile geometry clean", "random area cases clean", "edge area cases clean"])
