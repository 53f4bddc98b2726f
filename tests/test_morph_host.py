"""Erode / dilate / morphological gradient (mi_blur_cpu_run_morph, mi_blur_ctx_set_morph, erode() / dilate() /
morph_gradient(), the hosts' --erode / --dilate / --morph-gradient), CPU only: byte for byte against a numpy restatement of
the definition in include/mi_blur.h (morph_ref.py, which also says why the inputs are what they are), independent of the
product."""
import subprocess

import numpy as np
import pytest

from filter_harness import (MEDIAN, MORPH, SEP, apps, check_cpu_band_split_equals_whole, check_cpu_context, check_set_rules_order,  # noqa: F401
                            cpu_run, read_ppm, write_ppm)
from morph_ref import DILATE, ERODE, GRADIENT, OPS, corner_impulses, ref_morph, ref_morph_2d, structured


def inputs(rng, n, h, w, c, small):
    out = [corner_impulses(h, w, c)] + structured(rng, n, h, w, c, sparse_and_constant=True)
    if small:
        out.append(rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8))
    return out


def cpu_morph(pkg, L, img, op, rx, ry, n_threads=3):
    return cpu_run(MORPH, pkg, L, img, (op, rx, ry), n_threads)


# ---------------------------------------------------------------- the yardstick itself
def test_separable_restatement_is_the_2d_definition():
    rng = np.random.default_rng(0)
    for (n, h, w, c) in ((1, 1, 1, 2), (2, 9, 13, 3), (1, 40, 37, 1), (1, 5, 45, 2)):
        for img in inputs(rng, n, h, w, c, True):
            for rx in (0, 1, 2, 5, 16):
                for ry in (0, 1, 2, 5, 16):
                    for op in OPS:
                        assert np.array_equal(ref_morph(img, op, rx, ry), ref_morph_2d(img, op, rx, ry)), ((n, h, w, c), op, rx, ry)


def test_impulses_paint_exact_rectangles():
    """What the impulse images are for, checked on the restatement: one rectangle of (2rx+1) x (2ry+1), one channel."""
    img = np.full((1, 80, 90, 3), 128, np.uint8)
    img[0, 40, 50, 1] = 255
    d = ref_morph(img, DILATE, 4, 2)
    want = np.full_like(img, 128)
    want[0, 38:43, 46:55, 1] = 255
    assert np.array_equal(d, want)
    assert np.array_equal(ref_morph(img, ERODE, 4, 2), np.full_like(img, 128))


# ---------------------------------------------------------------- mi_blur_cpu_run_morph
SHAPES = [(1, 1, 1, 3), (1, 1, 40, 3), (1, 37, 1, 1), (2, 5, 6, 4), (1, 9, 11, 5), (2, 17, 33, 3), (1, 24, 64, 1),
          (1, 21, 16, 8), (3, 12, 13, 2)]
RADII = (0, 1, 2, 3, 4, 7, 8, 15, 16)


def test_cpu_run_morph_all_radii(pkg, L):
    """Every (rx, ry) of RADII squared on impulses and low-amplitude noise, 1 and 4 threads."""
    rng = np.random.default_rng(1)
    for (n, h, w, c) in ((2, 17, 33, 3), (1, 45, 50, 1), (1, 38, 36, 4)):
        imgs = [corner_impulses(h, w, c), rng.integers(100, 141, size=(n, h, w, c), dtype=np.uint8)]
        for rx in RADII:
            for ry in RADII:
                for op in OPS:
                    for k, img in enumerate(imgs):
                        want = ref_morph(img, op, rx, ry)
                        for nt in (1, 4):
                            assert np.array_equal(cpu_morph(pkg, L, img, op, rx, ry, nt), want), ((n, h, w, c), op, rx, ry, k, nt)


def test_cpu_run_morph_shapes(pkg, L):
    rng = np.random.default_rng(2)
    pairs = [(0, 0), (1, 1), (2, 2), (0, 3), (3, 0), (4, 1), (2, 7), (8, 8), (15, 4), (7, 16), (16, 16)]
    for (n, h, w, c) in SHAPES:
        for rx, ry in pairs:
            for img in inputs(rng, n, h, w, c, max(rx, ry) <= 2):
                for op in OPS:
                    want = ref_morph(img, op, rx, ry)
                    for nt in (1, 4):
                        assert np.array_equal(cpu_morph(pkg, L, img, op, rx, ry, nt), want), ((n, h, w, c), op, rx, ry, nt)


def test_cpu_run_morph_identity_radius(pkg, L):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(2, 11, 14, 3), dtype=np.uint8)
    assert np.array_equal(cpu_morph(pkg, L, img, ERODE, 0, 0), img)
    assert np.array_equal(cpu_morph(pkg, L, img, DILATE, 0, 0), img)
    assert not cpu_morph(pkg, L, img, GRADIENT, 0, 0).any()


def test_cpu_run_morph_refusals(pkg, L):
    a = np.zeros((8, 8, 3), np.uint8)
    b = np.zeros_like(a)
    A, B = a.ctypes.data, b.ctypes.data
    assert L.mi_blur_cpu_run_morph(A, B, 8, 8, 3, ERODE, 1, 1, 1, 1) == pkg.OK
    assert L.mi_blur_cpu_run_morph(A, B, 8, 8, 3, GRADIENT, 16, 0, 0, 1) == pkg.OK           # n_images == 0
    for op in (-1, 3, 100):
        assert L.mi_blur_cpu_run_morph(A, B, 8, 8, 3, op, 1, 1, 1, 1) == pkg.ERR_INVALID, op
    for rx, ry in ((-1, 1), (1, -1), (17, 1), (1, 17), (100, 100)):
        assert L.mi_blur_cpu_run_morph(A, B, 8, 8, 3, DILATE, rx, ry, 1, 1) == pkg.ERR_INVALID, (rx, ry)
    for args in [(A, A, 8, 8, 3, ERODE, 1, 1, 1), (A, B, 0, 8, 3, ERODE, 1, 1, 1), (A, B, 8, 0, 3, ERODE, 1, 1, 1),
                 (A, B, 8, 8, 0, ERODE, 1, 1, 1), (A, B, 8, 8, 3, ERODE, 1, 1, -1), (None, B, 8, 8, 3, ERODE, 1, 1, 1),
                 (A, None, 8, 8, 3, ERODE, 1, 1, 1)]:
        assert L.mi_blur_cpu_run_morph(*args, 1) == pkg.ERR_INVALID, args
    assert pkg.MORPH_MAX_RADIUS == 16
    assert (pkg.MORPH_ERODE, pkg.MORPH_DILATE, pkg.MORPH_GRADIENT) == OPS


def test_enqueue_morph_without_a_device(pkg, L):
    a = np.zeros((8, 16, 3), np.uint8)
    b = np.zeros_like(a)
    A, B = a.ctypes.data, b.ctypes.data
    # argument errors come before MI_BLUR_ERR_NO_DEVICE, so they read the same with and without a GPU
    assert L.mi_blur_enqueue_morph(A, B, 16, 8, 3, 3, 1, 1, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph(A, B, 16, 8, 3, ERODE, 17, 1, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph(A, B, 16, 8, 3, ERODE, 1, -1, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph(A, A, 16, 8, 3, ERODE, 1, 1, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph(A, B, 16, 8, 3, ERODE, 1, 1, -1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph_band(A, B, 16, 8, 3, -1, 1, 1, 2, 6, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph_band(A, B, 0, 8, 3, DILATE, 1, 1, 2, 6, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph_band(None, B, 16, 8, 3, DILATE, 1, 1, 2, 6, None) == pkg.ERR_INVALID
    if L.mi_blur_device_count() > 0:
        return                                                   # with a device the GPU tests cover the rest
    assert L.mi_blur_enqueue_morph(A, B, 16, 8, 3, ERODE, 1, 1, 1, None) == pkg.ERR_NO_DEVICE
    assert L.mi_blur_enqueue_morph(A, B, 16, 8, 3, ERODE, 1, 1, 0, None) == pkg.ERR_NO_DEVICE
    assert L.mi_blur_enqueue_morph_band(A, B, 16, 8, 3, GRADIENT, 2, 2, 2, 6, None) == pkg.ERR_NO_DEVICE


# ---------------------------------------------------------------- CPU-device context
def test_cpu_context_with_a_morph(pkg, L):
    rng = np.random.default_rng(11)
    n, h, w, c = 4, 37, 41, 3
    img = rng.integers(100, 141, size=(n, h, w, c), dtype=np.uint8)
    img[0] = corner_impulses(h, w, c)[0]
    for filt in ((ERODE, 1, 1), (DILATE, 5, 3), (GRADIENT, 2, 4), (ERODE, 16, 0)):
        check_cpu_context(MORPH, pkg, L, img, filt, dict(n_slots=2, n_threads=3))


def test_band_split_with_halo_ry_equals_whole(pkg, L):
    rng = np.random.default_rng(12)
    h, w, c = 75, 23, 3
    img = rng.integers(100, 141, size=(1, h, w, c), dtype=np.uint8)
    img[0, ::9, ::7, 1] = 255
    img[0, 4::9, 3::7, 2] = 0
    for op, rx, ry in ((ERODE, 2, 1), (DILATE, 1, 5), (GRADIENT, 3, 16), (DILATE, 4, 0)):
        splits = (max(ry, 1), h // 3, h // 2, h - max(ry, 1))
        check_cpu_band_split_equals_whole(MORPH, pkg, L, img, (op, rx, ry), splits, dict(n_threads=2))


def test_set_morph_rules(pkg, L):
    """A context holds one filter: set_kernel, set_median and set_morph each replace what another set before."""
    rng = np.random.default_rng(13)
    img = rng.integers(100, 141, size=(2, 20, 24, 3), dtype=np.uint8)
    kern, med, mor = (SEP, pkg.gauss_kernel(2.0)), (MEDIAN, 2), (MORPH, (DILATE, 3, 1))
    check_set_rules_order(MORPH, pkg, L, img,
                          [(kern, mor), (med, mor), (kern, med, mor), (mor, (MORPH, (ERODE, 0, 2))), (mor, med), (mor, kern),
                           (med, mor, kern), (kern, mor, med)],
                          refused=[(-1, 1, 1), (3, 1, 1), (ERODE, -1, 0), (ERODE, 0, 17), (DILATE, 17, 17)], good=(ERODE, 1, 1))


# ---------------------------------------------------------------- Python functions
def test_morphology_functions_on_the_cpu_device(pkg):
    rng = np.random.default_rng(5)
    img = rng.integers(100, 141, size=(40, 50, 3), dtype=np.uint8)
    img[7, 9, 0] = 255
    img[39, 49, 2] = 0
    fns = ((pkg.erode, ERODE), (pkg.dilate, DILATE), (pkg.morph_gradient, GRADIENT))
    for fn, op in fns:
        for k in (1, 3, 5, 9, 33):
            got = fn(img, k, device=pkg.DEVICE_CPU)
            assert got.shape == img.shape and np.array_equal(got, ref_morph(img[None], op, k // 2, k // 2)[0]), (op, k)
        for kx, ky in ((3, 1), (1, 7), (33, 5), (5, 33)):
            assert np.array_equal(fn(img, (kx, ky), device=pkg.DEVICE_CPU), ref_morph(img[None], op, kx // 2, ky // 2)[0]), (op, kx, ky)
        g = img[:, :, 0]
        got = fn(g, [7, 3], device=pkg.DEVICE_CPU)
        assert got.shape == g.shape and np.array_equal(got, ref_morph(g[None, :, :, None], op, 3, 1)[0, :, :, 0])
        batch = rng.integers(0, 256, size=(3, 12, 10, 4), dtype=np.uint8)
        assert np.array_equal(fn(batch, 5, device=pkg.DEVICE_CPU, batch=2), ref_morph(batch, op, 2, 2))
        assert np.array_equal(fn(img, device=pkg.DEVICE_CPU), ref_morph(img[None], op, 1, 1)[0])      # ksize defaults to 3
        for bad in (0, 2, 4, 35, -3, (3, 4), (35, 3), (3,), (3, 3, 3), 3.0, "3", None):
            with pytest.raises(ValueError):
                fn(img, bad, device=pkg.DEVICE_CPU)
        with pytest.raises(ValueError):
            fn(img.astype(np.float32), 3, device=pkg.DEVICE_CPU)


# ---------------------------------------------------------------- hosts
def test_host_cpu_morph(apps, tmp_path):
    het, _ = apps
    rng = np.random.default_rng(9)
    img = rng.integers(100, 141, size=(45, 61, 3)).astype(np.uint8)
    img[0, 0, 0], img[44, 60, 1], img[20, 30, 2], img[21, 5, 0] = 255, 0, 255, 0
    write_ppm(tmp_path / "in.ppm", img)
    for flag, k, op, name in (("--erode", 5, ERODE, "erode"), ("--dilate", 9, DILATE, "dilate"),
                              ("--morph-gradient", 3, GRADIENT, "morphological gradient")):
        r = subprocess.run([het, "cpu", "0.5", "7", "--image", "in.ppm", "--images", "20", flag, str(k), "--save", "out.ppm"],
                           cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"Blur kernel: {k}x{k} {name}\n" in r.stdout
        assert np.array_equal(read_ppm(tmp_path / "out.ppm"), ref_morph(img[None], op, k // 2, k // 2)[0]), flag


def test_host_morph_refusals(apps, tmp_path):
    het, spl = apps
    syn = [het, "cpu", "--synthetic"]
    for cmd in (syn + ["--erode", "4"], syn + ["--erode", "35"], syn + ["--dilate", "1"], syn + ["--morph-gradient", "0"],
                syn + ["--erode"], syn + ["--erode", "5", "--dilate", "5"], syn + ["--dilate", "5", "--morph-gradient", "3"],
                syn + ["--erode", "5", "--erode", "5"], syn + ["--erode", "5", "--sigma", "2"], syn + ["--ksize", "3", "--dilate", "5"],
                syn + ["--median", "5", "--morph-gradient", "5"], syn + ["--erode", "5", "--median", "3"],
                [het, "gpu", "--erode", "3", "--resident"], [spl, "--resident", "--dilate", "3"],
                [spl, "--synthetic", "--morph-gradient", "6"]):
        r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Error:" in r.stdout, (cmd, r.stdout)
