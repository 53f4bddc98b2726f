"""Median blur (mi_blur_cpu_run_median, mi_blur_ctx_set_median, median_blur(), the hosts' --median), CPU only: against a
numpy restatement of the definition in include/mi_blur.h (median_ref.py), independent of the product."""
import subprocess

import numpy as np
import pytest

from filter_harness import MEDIAN, apps, check_cpu_band_split_equals_whole, check_cpu_context, cpu_run, read_ppm, write_ppm  # noqa: F401
from median_ref import adversarial, ref_median

# ---------------------------------------------------------------- mi_blur_cpu_run_median
SHAPES = [(1, 1, 1, 3), (1, 1, 40, 3), (1, 37, 1, 1), (2, 5, 6, 4), (1, 9, 11, 5), (2, 17, 33, 3), (1, 24, 64, 1),
          (1, 21, 16, 8), (3, 12, 13, 2)]


def test_cpu_run_median_random(pkg, L):
    rng = np.random.default_rng(1)
    for (n, h, w, c) in SHAPES:
        img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
        for r in range(1, 8):
            want = ref_median(img, r)
            for nt in (1, 4):
                assert np.array_equal(cpu_run(MEDIAN, pkg, L, img, r, nt), want), ((n, h, w, c), r, nt)


def test_cpu_run_median_adversarial(pkg, L):
    rng = np.random.default_rng(2)
    for (n, h, w, c) in ((1, 20, 32, 3), (2, 9, 7, 1), (1, 30, 17, 5)):
        for img in adversarial(rng, n, h, w, c):
            for r in (1, 2, 3, 7):
                assert np.array_equal(cpu_run(MEDIAN, pkg, L, img, r, 3), ref_median(img, r)), ((n, h, w, c), r)


def test_cpu_run_median_refusals(pkg, L):
    a = np.zeros((8, 8, 3), np.uint8)
    b = np.zeros_like(a)
    assert L.mi_blur_cpu_run_median(a.ctypes.data, b.ctypes.data, 8, 8, 3, 1, 1, 1) == pkg.OK
    for r in (0, -1, 8, 100):
        assert L.mi_blur_cpu_run_median(a.ctypes.data, b.ctypes.data, 8, 8, 3, r, 1, 1) == pkg.ERR_INVALID, r
    for args in [(a.ctypes.data, a.ctypes.data, 8, 8, 3, 1, 1), (a.ctypes.data, b.ctypes.data, 0, 8, 3, 1, 1),
                 (a.ctypes.data, b.ctypes.data, 8, 0, 3, 1, 1), (a.ctypes.data, b.ctypes.data, 8, 8, 0, 1, 1),
                 (a.ctypes.data, b.ctypes.data, 8, 8, 3, 1, -1), (None, b.ctypes.data, 8, 8, 3, 1, 1),
                 (a.ctypes.data, None, 8, 8, 3, 1, 1)]:
        assert L.mi_blur_cpu_run_median(*args, 1) == pkg.ERR_INVALID, args
    assert pkg.MEDIAN_MAX_RADIUS == 7


def test_enqueue_median_without_a_device(pkg, L):
    if L.mi_blur_device_count() > 0:
        pytest.skip("a HIP device is present: the GPU tests cover these entry points")
    a = np.zeros((8, 16, 3), np.uint8)
    b = np.zeros_like(a)
    assert L.mi_blur_enqueue_median(a.ctypes.data, b.ctypes.data, 16, 8, 3, 1, 1, None) == pkg.ERR_NO_DEVICE
    assert L.mi_blur_enqueue_median_band(a.ctypes.data, b.ctypes.data, 16, 8, 3, 2, 2, 6, None) == pkg.ERR_NO_DEVICE
    # argument errors come first
    assert L.mi_blur_enqueue_median(a.ctypes.data, b.ctypes.data, 16, 8, 3, 8, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_median(a.ctypes.data, a.ctypes.data, 16, 8, 3, 1, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_median_band(a.ctypes.data, b.ctypes.data, 16, 8, 3, 0, 2, 6, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_median_band(a.ctypes.data, b.ctypes.data, 0, 8, 3, 1, 2, 6, None) == pkg.ERR_INVALID


# ---------------------------------------------------------------- CPU-device context
def test_cpu_context_with_a_median(pkg, L):
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, size=(4, 37, 41, 3), dtype=np.uint8)
    for r in (1, 3):
        check_cpu_context(MEDIAN, pkg, L, img, r, dict(n_slots=2, n_threads=3))


def test_band_split_with_halo_r_equals_whole(pkg, L):
    rng = np.random.default_rng(12)
    h, w, c = 45, 23, 3
    img = rng.integers(0, 256, size=(1, h, w, c), dtype=np.uint8)
    for r in (1, 2, 5):
        check_cpu_band_split_equals_whole(MEDIAN, pkg, L, img, r, (r, h // 3, h // 2, h - r), dict(n_threads=2))


def test_set_median_rules(pkg, L):
    rng = np.random.default_rng(13)
    n, h, w, c = 2, 20, 24, 3
    img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    with pkg.Context(pkg.DEVICE_CPU, w, h, c, 1, max_batch=n) as ctx:
        for r in (0, -1, 8):
            assert L.mi_blur_ctx_set_median(ctx.h, r) == pkg.ERR_INVALID
        assert L.mi_blur_ctx_set_median(None, 1) == pkg.ERR_INVALID
        ctx.set_kernel(pkg.gauss_kernel(2.0))                                   # set_kernel, then set_median: the median
        ctx.set_median(2)
        out = np.zeros_like(img)
        ctx.submit(img.ctypes.data, out.ctypes.data, n)
        ctx.sync()
        assert np.array_equal(out, ref_median(img, 2))
    with pkg.Context(pkg.DEVICE_CPU, w, h, c, 1, max_batch=n) as ctx:
        ctx.set_median(2)                                                       # set_median, then set_kernel: the kernel
        k = pkg.SepKernel.from_taps([1, 2, 1])
        ctx.set_kernel(k)
        out = np.zeros_like(img)
        ctx.submit(img.ctypes.data, out.ctypes.data, n)
        ctx.sync()
        want = np.empty_like(img)
        assert L.mi_blur_cpu_run(img.ctypes.data, want.ctypes.data, w, h, c, 1, n, 1) == pkg.OK
        assert np.array_equal(out, want)


def test_median_blur_on_the_cpu_device(pkg):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(30, 50, 3), dtype=np.uint8)
    for k in (3, 5, 9, 15):
        assert np.array_equal(pkg.median_blur(img, k, device=pkg.DEVICE_CPU), ref_median(img[None], k // 2)[0]), k
    g = img[:, :, 0]
    assert np.array_equal(pkg.median_blur(g, 7, device=pkg.DEVICE_CPU), ref_median(g[None, :, :, None], 3)[0, :, :, 0])
    batch = rng.integers(0, 256, size=(3, 12, 10, 4), dtype=np.uint8)
    assert np.array_equal(pkg.median_blur(batch, 5, device=pkg.DEVICE_CPU, batch=2), ref_median(batch, 2))
    for bad in (1, 2, 4, 17):
        with pytest.raises(ValueError):
            pkg.median_blur(img, bad, device=pkg.DEVICE_CPU)


# ---------------------------------------------------------------- hosts
def test_host_cpu_median(apps, tmp_path):
    het, _ = apps
    rng = np.random.default_rng(9)
    img = np.where(rng.random((45, 61, 3)) < 0.1, rng.choice([0, 255], (45, 61, 3)),
                   rng.integers(60, 190, size=(45, 61, 3))).astype(np.uint8)
    write_ppm(tmp_path / "in.ppm", img)
    r = subprocess.run([het, "cpu", "0.5", "7", "--image", "in.ppm", "--images", "20", "--median", "5", "--save", "out.ppm"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Blur kernel: 5x5 median" in r.stdout
    assert np.array_equal(read_ppm(tmp_path / "out.ppm"), ref_median(img[None], 2)[0])


def test_host_median_refusals(apps, tmp_path):
    het, spl = apps
    for cmd in ([het, "cpu", "--synthetic", "--median", "4"], [het, "cpu", "--synthetic", "--median", "17"],
                [het, "cpu", "--synthetic", "--median", "1"], [het, "cpu", "--synthetic", "--median", "5", "--sigma", "2"],
                [het, "cpu", "--synthetic", "--median", "5", "--ksize", "3"], [het, "gpu", "--median", "3", "--resident"],
                [spl, "--resident", "--median", "3"]):
        r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Error:" in r.stdout, (cmd, r.stdout)
