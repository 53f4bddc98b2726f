"""The decimating separable filter (mi_blur_decimated_size, mi_blur_sep_down_preset, mi_blur_cpu_run_sep_down,
mi_blur_ctx_set_sep_down, pyr_down / area_down / sep_down), CPU only: against sep_ref.ref_sep followed by the subsampling
(sep_down_ref.py), independent of the product.  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest

from filter_harness import MEDIAN, cpu_run as cpu_run_same_size
from resample_harness import (SEP_DOWN, check_cpu_context, check_cpu_run_refuses, check_enqueue_invalid_before_no_device, check_setters_replace_each_other,
                              cpu_run, no_scratch)
from sep_down_ref import PHASES, PRESETS, down_shape, ref_sep_down
from sep_ref import rand_taps, ref_sep

SHAPES = [(3, 33, 40, 3), (1, 1, 1, 3), (2, 9, 5, 1), (1, 17, 16, 4), (1, 50, 7, 5), (1, 64, 96, 2)]
RADII = [(0, 0), (1, 1), (3, 5), (16, 16), (0, 4)]


def preset(pkg, L, which):
    k, d = pkg.SepKernel(), pkg.Decimation()
    assert L.mi_blur_sep_down_preset(which, C.byref(k), C.byref(d)) == pkg.OK
    return k, (d.sx, d.sy, d.ox, d.oy)


def test_decimated_size_matches_the_formula(pkg, L):
    wo, ho = C.c_int(), C.c_int()
    for w in range(1, 10):
        for h in range(1, 10):
            for sx, sy, ox, oy in PHASES:
                d = pkg.Decimation(sx, sy, ox, oy)
                rc = L.mi_blur_decimated_size(w, h, C.byref(d), C.byref(wo), C.byref(ho))
                if ox >= w or oy >= h:
                    assert rc == pkg.ERR_INVALID, (w, h, sx, sy, ox, oy)
                    continue
                assert rc == pkg.OK
                assert (wo.value, ho.value) == ((w - ox + sx - 1) // sx, (h - oy + sy - 1) // sy), (w, h, sx, sy, ox, oy)
                assert (wo.value, ho.value) == (len(range(ox, w, sx)), len(range(oy, h, sy)))
                assert pkg.decimated_size(w, h, sx, sy, ox, oy) == (wo.value, ho.value)
    d = pkg.Decimation(2, 2, 0, 0)
    assert L.mi_blur_decimated_size(8, 8, None, C.byref(wo), C.byref(ho)) == pkg.ERR_INVALID
    assert L.mi_blur_decimated_size(8, 8, C.byref(d), None, C.byref(ho)) == pkg.ERR_INVALID
    assert L.mi_blur_decimated_size(0, 8, C.byref(d), C.byref(wo), C.byref(ho)) == pkg.ERR_INVALID


def bad_rows(pkg):
    """(good, rows) for resample_harness.bad_calls: the strides, phases and taps the header calls invalid."""
    good_k, good_d = pkg.SepKernel.from_taps([1, 2, 1]), pkg.Decimation(2, 2, 0, 0)
    row = lambda w, h, k, d: (w, h, 3, (C.byref(k), C.byref(d)))
    rows = [row(8, 8, good_k, pkg.Decimation(*dec))
            for dec in [(0, 2, 0, 0), (2, 0, 0, 0), (5, 2, 0, 0), (2, 5, 0, 0), (2, 2, 2, 0), (2, 2, 0, 2), (3, 3, 3, 1), (2, 2, -1, 0), (2, 2, 0, -1)]]
    rows.append(row(2, 8, good_k, pkg.Decimation(4, 1, 2, 0)))      # ox >= W
    rows.append(row(8, 3, good_k, pkg.Decimation(1, 4, 0, 3)))      # oy >= H
    k = pkg.SepKernel.from_taps([1, 2, 1]); k.wx[0] = 2; rows.append(row(8, 8, k, good_d))     # sum 5
    k = pkg.SepKernel.from_taps([1, 2, 1]); k.rx = 17; rows.append(row(8, 8, k, good_d))
    k = pkg.SepKernel.from_taps([1, 2, 1]); k.by = 3; rows.append(row(8, 8, k, good_d))
    return (C.byref(good_k), C.byref(good_d)), rows


def test_cpu_run_refuses_invalid_arguments(pkg, L):
    check_cpu_run_refuses(SEP_DOWN, pkg, L, *bad_rows(pkg))


def test_enqueue_invalid_comes_before_no_device(pkg, L):
    """Every argument is checked before a device is asked for; without a GPU a good call is ERR_NO_DEVICE (with one, the
    null stream of an empty batch is MI_BLUR_OK)."""
    check_enqueue_invalid_before_no_device(SEP_DOWN, pkg, L, *bad_rows(pkg))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cpu_run_matches_the_reference(pkg, L, shape):
    """Every stride pair in 1..4, every valid phase, five radius pairs, 1 and 4 threads; the filtered image is restated once
    per taps and subsampled per phase."""
    rng = np.random.default_rng(sum(shape))
    img = rng.integers(0, 256, size=shape, dtype=np.uint8)
    n, h, w, c = shape
    for rx, ry in RADII:
        wx, wy = rand_taps(rng, rx), rand_taps(rng, ry, bits=6)
        full = ref_sep(img, wx, wy)
        k = pkg.SepKernel.from_taps(wx, wy)
        for dec in PHASES:
            sx, sy, ox, oy = dec
            if ox >= w or oy >= h:
                continue
            want = full[:, oy::sy, ox::sx, :]
            assert want.shape == down_shape(shape, *dec)
            for nt in (1, 4):
                assert np.array_equal(cpu_run(SEP_DOWN, pkg, L, img, (k, dec), nt), want), (shape, rx, ry, dec, nt)


def test_stride_one_is_the_separable_filter(pkg, L):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(2, 21, 19, 3), dtype=np.uint8)
    k = pkg.SepKernel.from_taps(rand_taps(rng, 3), rand_taps(rng, 2))
    full = np.empty_like(img)
    assert L.mi_blur_cpu_run_sep(img.ctypes.data, full.ctypes.data, 19, 21, 3, 2, C.byref(k), 2) == pkg.OK
    assert np.array_equal(cpu_run(SEP_DOWN, pkg, L, img, (k, (1, 1, 0, 0)), 2), full)


def test_presets(pkg, L):
    for which, (taps, stride) in PRESETS.items():
        k, dec = preset(pkg, L, which)
        assert k.taps() == (taps, taps) and dec == (stride, stride, 0, 0), which
    k, d = pkg.SepKernel(), pkg.Decimation()
    for which in (-1, 3):
        assert L.mi_blur_sep_down_preset(which, C.byref(k), C.byref(d)) == pkg.ERR_INVALID
    assert L.mi_blur_sep_down_preset(0, None, C.byref(d)) == pkg.ERR_INVALID
    assert L.mi_blur_sep_down_preset(0, C.byref(k), None) == pkg.ERR_INVALID
    # AREA2 / AREA4 on an image of constant blocks: the block values; on a random one: the truncated block means
    rng = np.random.default_rng(11)
    for which, f in ((1, 2), (2, 4)):
        k, dec = preset(pkg, L, which)
        blocks = rng.integers(0, 256, size=(2, 6, 5, 3), dtype=np.uint8)
        img = np.repeat(np.repeat(blocks, f, axis=1), f, axis=2)
        assert np.array_equal(cpu_run(SEP_DOWN, pkg, L, img, (k, dec), 2), blocks)
        img = rng.integers(0, 256, size=(2, 6 * f, 5 * f, 3), dtype=np.uint8)
        means = img.reshape(2, 6, f, 5, f, 3).astype(np.int64).sum(axis=(2, 4)) // (f * f)
        assert np.array_equal(cpu_run(SEP_DOWN, pkg, L, img, (k, dec), 2), means.astype(np.uint8))
        assert np.array_equal(ref_sep_down(img, *k.taps(), *dec), means.astype(np.uint8))


def test_cpu_context(pkg, L):
    rng = np.random.default_rng(23)
    img = rng.integers(0, 256, size=(5, 37, 42, 3), dtype=np.uint8)
    n, h, w, c = img.shape
    wx, wy = rand_taps(rng, 3), rand_taps(rng, 5)
    dec = (2, 3, 1, 2)
    check_cpu_context(SEP_DOWN, pkg, L, img, (pkg.SepKernel.from_taps(wx, wy), dec))
    with pkg.Context(pkg.DEVICE_CPU, w, h, c, 1, max_batch=n) as ctx:     # refused sets leave the context as it was
        good = pkg.SepKernel.from_taps(wx, wy)
        assert L.mi_blur_ctx_set_sep_down(None, C.byref(good), C.byref(pkg.Decimation(*dec))) == pkg.ERR_INVALID
        assert L.mi_blur_ctx_set_sep_down(ctx.h, None, C.byref(pkg.Decimation(*dec))) == pkg.ERR_INVALID
        assert L.mi_blur_ctx_set_sep_down(ctx.h, C.byref(good), None) == pkg.ERR_INVALID
        assert L.mi_blur_ctx_set_sep_down(ctx.h, C.byref(good), C.byref(pkg.Decimation(5, 2, 0, 0))) == pkg.ERR_INVALID
        out = np.empty_like(img)
        ctx.submit(img.ctypes.data, out.ctypes.data, n)
        t = ctx.sync()
        box = np.empty_like(img)
        assert L.mi_blur_cpu_run(img.ctypes.data, box.ctypes.data, w, h, c, 1, n, 1) == pkg.OK
        assert np.array_equal(out, box) and t["bytes_alg"] == 2 * img.size


def test_setters_replace_each_other(pkg, L):
    rng = np.random.default_rng(29)
    img = rng.integers(0, 256, size=(2, 20, 24, 3), dtype=np.uint8)
    k = pkg.SepKernel.from_taps(rand_taps(rng, 2), rand_taps(rng, 1))
    down = lambda ctx: ctx.set_sep_down(k, 2, 2, 1, 0)
    median = lambda ctx: ctx.set_median(1)
    med, dec = cpu_run_same_size(MEDIAN, pkg, L, img, 1, 1), ref_sep_down(img, *k.taps(), 2, 2, 1, 0)
    check_setters_replace_each_other(pkg, L, img, [([down, median], med), ([median, down], dec)])      # the last one wins: the median at full size


def test_numpy_functions_on_the_cpu_device(pkg, L):
    rng = np.random.default_rng(31)
    stack = rng.integers(0, 256, size=(4, 45, 71, 3), dtype=np.uint8)
    pyr, a2, a4 = (PRESETS[i] for i in range(3))
    for img in (stack, stack[0], np.ascontiguousarray(stack[0, :, :, 0])):
        as4 = img if img.ndim == 4 else img[None] if img.ndim == 3 else img[None, :, :, None]
        shape = lambda want: want.reshape(want.shape if img.ndim == 4 else want.shape[1:] if img.ndim == 3 else want.shape[1:3])
        got = pkg.pyr_down(img, device=pkg.DEVICE_CPU, batch=3)
        want = shape(ref_sep_down(as4, pyr[0], pyr[0]))
        assert got.shape == want.shape and got.ndim == img.ndim and np.array_equal(got, want)
        assert got.shape[-3 if img.ndim > 2 else -2:][:2] == (23, 36)
        assert np.array_equal(pkg.area_down(img, device=pkg.DEVICE_CPU, batch=3), shape(ref_sep_down(as4, a2[0], a2[0])))
        assert np.array_equal(pkg.area_down(img, 4, device=pkg.DEVICE_CPU), shape(ref_sep_down(as4, a4[0], a4[0], 4, 4)))
        wx, wy = rand_taps(rng, 4), rand_taps(rng, 2)
        got = pkg.sep_down(img, pkg.SepKernel.from_taps(wx, wy), 3, 2, 2, 1, device=pkg.DEVICE_CPU, batch=3)
        assert np.array_equal(got, shape(ref_sep_down(as4, wx, wy, 3, 2, 2, 1)))
    empty = pkg.pyr_down(np.zeros((0, 45, 71, 3), np.uint8), device=pkg.DEVICE_CPU)
    assert empty.shape == (0, 23, 36, 3) and empty.dtype == np.uint8
    with pytest.raises(ValueError):
        pkg.area_down(stack, 3, device=pkg.DEVICE_CPU)
    with pytest.raises(ValueError):
        pkg.pyr_down(stack.astype(np.float32), device=pkg.DEVICE_CPU)
    with pytest.raises(pkg.MiBlurError):
        pkg.sep_down(stack, pkg.SepKernel.from_taps([1, 2, 1]), 5, 2, device=pkg.DEVICE_CPU)


def test_tiled_kernels_use_no_scratch(pkg, tmp_path):
    """Compiles sep_down_kernels.hip to gfx950 assembly (no GPU needed): the gather of the horizontal pass is all
    compile-time positions, so no tiled instantiation may spill or index registers at run time."""
    no_scratch(pkg, tmp_path, "sep_down_kernels.hip", "blur_sep_down_tiled_kernel", 12)      # 4 channel counts x 3 radius buckets
