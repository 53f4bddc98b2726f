"""Median blur on a real MI355X (-m gpu): mi_blur_enqueue_median / _band, a context given a median by
mi_blur_ctx_set_median, median_blur() and the hosts' --median, byte for byte against a numpy restatement of the definition
in include/mi_blur.h (median_ref.py: edge padding, sliding windows, np.partition) and against the CPU device."""
import subprocess

import numpy as np
import pytest

from filter_harness import (MEDIAN, apps, check_batch_over_2gib, check_bands_inside_the_image, check_gpu_context,  # noqa: F401
                            check_synthetic_stream, check_unaligned_pointers, gpu_run, read_ppm, torch_cuda, write_ppm)
from median_ref import adversarial, ref_median

pytestmark = pytest.mark.gpu

# rows of whole 16-byte chunks with 1-4 channels (the fast kernel at radius 1|2) and everything else
ALIGNED = [(2, 64, 80, 3), (1, 40, 64, 4), (3, 33, 16, 1), (1, 100, 1024, 1), (1, 37, 2000, 4), (2, 70, 96, 2),
           (1, 1, 16, 1), (1, 2, 48, 1), (1, 300, 512, 3), (1, 5, 32, 2)]
RAGGED = [(1, 17, 33, 3), (2, 30, 250, 3), (1, 9, 5, 1), (1, 31, 29, 2), (1, 50, 7, 5), (1, 24, 64, 5), (1, 1, 1, 3),
          (1, 12, 16, 6), (1, 10, 20, 7), (1, 14, 18, 8)]


def test_enqueue_median_matches_numpy(pkg, L, torch_cuda):
    rng = np.random.default_rng(2024)
    for shapes, aligned in ((ALIGNED, True), (RAGGED, False)):
        for (n, h, w, c) in shapes:
            img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
            for r in range(1, 8):
                got = gpu_run(MEDIAN, pkg, L, torch_cuda, img, r)
                assert L.mi_blur_last_kernel().decode() == MEDIAN.kernel(r, aligned), ((n, h, w, c), r)
                assert np.array_equal(got, ref_median(img, r)), ((n, h, w, c), r)


def test_enqueue_median_unaligned_pointers(pkg, L, torch_cuda):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(2, 40, 64, 3), dtype=np.uint8)
    for r in (1, 2):
        check_unaligned_pointers(MEDIAN, pkg, L, torch_cuda, img, r)


def test_enqueue_median_adversarial(pkg, L, torch_cuda):
    rng = np.random.default_rng(9)
    for (n, h, w, c) in ((1, 48, 64, 3), (2, 20, 48, 4), (1, 19, 16, 1), (1, 19, 30, 3), (1, 13, 11, 5)):
        for img in adversarial(rng, n, h, w, c):
            for r in (1, 2, 3, 7):
                assert np.array_equal(gpu_run(MEDIAN, pkg, L, torch_cuda, img, r), ref_median(img, r)), ((n, h, w, c), r)


def test_bands_inside_the_image(pkg, L, torch_cuda):
    rng = np.random.default_rng(12)
    for (h, w, c) in ((64, 80, 3), (37, 17, 3), (50, 64, 4), (40, 48, 1)):
        img = rng.integers(0, 256, size=(1, h, w, c), dtype=np.uint8)
        for r in (1, 2, 4, 7):
            check_bands_inside_the_image(MEDIAN, pkg, L, torch_cuda, img, r)


def test_enqueue_median_refusals(pkg, L, torch_cuda):
    d = torch_cuda.zeros(4096, dtype=torch_cuda.uint8, device="cuda")
    p, q = d.data_ptr(), d.data_ptr() + 2048
    for r in (0, 8, -1):
        assert L.mi_blur_enqueue_median(p, q, 16, 8, 3, r, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_median(p, p, 16, 8, 3, 1, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_median(p, q, 0, 8, 3, 1, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_median_band(p, q, 16, 8, 3, 1, 6, 2, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_median_band(p, q, 16, 8, 3, 1, 0, 9, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_median(p, q, 16, 8, 3, 1, 0, None) == pkg.OK


def test_batch_over_2gib(pkg, L, torch_cuda):
    """A batch of more than 2^31 bytes: 64-bit image offsets, the last image checked."""
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, size=(1, 1024, 1024, 3), dtype=np.uint8)
    n = 720                                                   # 2.26 GB in, as much out
    check_batch_over_2gib(MEDIAN, pkg, L, torch_cuda, img, (1, 2), n, same=(0, n // 2, n - 2))


def test_gpu_and_cpu_agree_on_the_synthetic_stream(pkg, L, torch_cuda):
    check_synthetic_stream(MEDIAN, pkg, L, torch_cuda, (1, 2), (1000, 256, 256, 3), fill_threads=8, cpu_threads=16)


def test_context_with_a_median(pkg, L, torch_cuda):
    """Every submit form of a GPU context takes the median: pageable, pinned (one launch: not the batch server), strided
    bands, one band, planar."""
    rng = np.random.default_rng(21)
    n, h, w, c = 6, 240, 320, 3                                # 1.38 MB of output per submit: the server size class
    img = np.where(rng.random((n, h, w, c)) < 0.1, rng.choice([0, 255], (n, h, w, c)),
                   rng.integers(0, 256, size=(n, h, w, c))).astype(np.uint8)
    for r in (1, 2, 4):
        check_gpu_context(MEDIAN, pkg, L, img, r, pinned_repeats=2)


def test_median_blur_python(pkg, torch_cuda):
    rng = np.random.default_rng(30)
    imgs = rng.integers(0, 256, size=(4, 90, 128, 3), dtype=np.uint8)
    for k in (3, 5, 7, 15):
        assert np.array_equal(pkg.median_blur(imgs, k), ref_median(imgs, k // 2)), k
    g = imgs[0, :, :, 0]
    assert np.array_equal(pkg.median_blur(g, 5), ref_median(g[None, :, :, None], 2)[0, :, :, 0])


def test_hosts_median_on_the_gpu(apps, torch_cuda, tmp_path):
    het, spl = apps
    rng = np.random.default_rng(40)
    img = np.where(rng.random((240, 320, 3)) < 0.1, rng.choice([0, 255], (240, 320, 3)),
                   rng.integers(0, 256, size=(240, 320, 3))).astype(np.uint8)
    write_ppm(tmp_path / "in.ppm", img)
    for k in (3, 5):
        want = ref_median(img[None], k // 2)[0]
        for mode in ("gpu", "both"):
            out = f"{mode}{k}.ppm"
            r = subprocess.run([het, mode, "0.7", "35", "--image", "in.ppm", "--images", "100", "--median", str(k), "--save", out],
                               cwd=tmp_path, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout + r.stderr
            assert f"Blur kernel: {k}x{k} median" in r.stdout
            assert np.array_equal(read_ppm(tmp_path / out), want), (mode, k)
    r = subprocess.run([spl, "0.6", "16", "--image", "in.ppm", "--images", "48", "--median", "5", "--save", "s.ppm"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Halo size: 2 row(s)" in r.stdout and "Blur kernel: 5x5 median" in r.stdout
    assert np.array_equal(read_ppm(tmp_path / "s.ppm"), ref_median(img[None], 2)[0])
