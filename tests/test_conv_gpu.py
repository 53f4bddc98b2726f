"""Signed 2-D convolution on a real MI355X (-m gpu): mi_blur_enqueue_conv / _band, a context given the filter by
mi_blur_ctx_set_conv, filter2d() / sobel() / ... and the hosts' --conv, byte for byte against the numpy restatement of the
definition in include/mi_blur.h (conv_ref.py) and against the CPU device.  0x5A guard bytes surround every output."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import conv_ref as cr
from conv_ref import ref_conv
from filter_harness import (CONV, TILE_CHUNKS, TILE_ROWS, apps, check_batch_over_2gib, check_bands_inside_the_image, check_gpu_context,  # noqa: F401
                            check_synthetic_stream, check_unaligned_pointers, cpu_run, gpu_run, read_ppm, seam_image, torch_cuda, write_ppm)

pytestmark = pytest.mark.gpu

TILED, GENERIC = CONV.fast, CONV.generic
# every rx (the column classes are 0-1, 2, 3, 4-5, 6-7) with a spread of ry
PAIRS = [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (7, 7), (0, 3), (1, 7), (2, 0), (3, 5), (4, 1), (5, 2), (6, 4), (7, 6)]
SOBEL_X = [[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]]
SOBEL = dict(K=SOBEL_X, mode="mag", K2=np.array(SOBEL_X).T.tolist())
SHARPEN = dict(K=[[0, -1, 0], [-1, 5, -1], [0, -1, 0]])


# rows of whole 16-byte chunks with 1-4 channels (the tiled kernel at every radius pair) and everything else
ALIGNED = {1: (2, 70, 1040), 2: (1, 65, 536), 3: (2, 66, 688), 4: (1, 40, 272)}        # c -> (n, h, w): several tiles both ways
RAGGED = [(1, 17, 33, 3), (2, 30, 250, 3), (1, 9, 5, 1), (1, 31, 29, 2), (1, 50, 7, 5), (1, 24, 64, 5), (1, 1, 1, 3), (1, 12, 16, 6), (1, 3, 15, 1)]


def test_tiled_kernel_every_radius_pair_channel_count_and_mode(pkg, L, torch_cuda):
    rng = np.random.default_rng(2024)
    assert {p[0] for p in PAIRS} == set(range(8)) and {p[1] for p in PAIRS} == set(range(8))
    for c, (n, h, w) in ALIGNED.items():
        imgs = [rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8), seam_image(rng, h, w, c)]
        for (rx, ry) in PAIRS:
            for mode in cr.MODES:
                spec = cr.random_kernel(rng, rx, ry, zeros=0.2, mode=mode)
                k = cr.make_kernel(pkg, **spec)
                for q, img in enumerate(imgs):
                    got = gpu_run(CONV, pkg, L, torch_cuda, img, k)
                    assert L.mi_blur_last_kernel().decode() == TILED, (c, rx, ry)
                    assert np.array_equal(got, ref_conv(img, **spec)), (c, rx, ry, mode, q)
                    assert np.array_equal(got, cpu_run(CONV, pkg, L, img, k, 8, prefill=False)), (c, rx, ry, mode, q)


def test_tile_edges(pkg, L, torch_cuda):
    """Heights and widths around the tile's row and chunk-column counts (one less, equal, one more, two tiles plus one)."""
    rng = np.random.default_rng(8)
    for c in (1, 3):
        for a, h in enumerate((TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, 2 * TILE_ROWS + 1)):
            for b, chunks in enumerate((TILE_CHUNKS - 1, TILE_CHUNKS, TILE_CHUNKS + 1, 2 * TILE_CHUNKS + 1)):
                w = chunks * 16                                  # cpr = chunks * c: rows of whole chunks whatever the channel count
                img = seam_image(rng, h, w, c)
                for (rx, ry, mode) in (((1, 1, "mag"), (4, 7, "sat"), (7, 2, "abs")), ((2, 3, "sat"), (5, 5, "mag")),
                                       ((3, 6, "abs"), (6, 1, "sat")), ((7, 7, "mag"), (0, 4, "abs")))[(a + b) % 4]:
                    spec = cr.random_kernel(rng, rx, ry, zeros=0.2, mode=mode)
                    got = gpu_run(CONV, pkg, L, torch_cuda, img, cr.make_kernel(pkg, **spec))
                    assert L.mi_blur_last_kernel().decode() == TILED
                    assert np.array_equal(got, ref_conv(img, **spec)), (h, w, c, rx, ry, mode)


def test_generic_kernel(pkg, L, torch_cuda):
    rng = np.random.default_rng(4)
    for (n, h, w, c) in RAGGED:
        img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
        for q, (rx, ry) in enumerate(PAIRS):
            spec = cr.random_kernel(rng, rx, ry, zeros=0.3 * (q % 2), mode=cr.MODES[q % 3])
            got = gpu_run(CONV, pkg, L, torch_cuda, img, cr.make_kernel(pkg, **spec))
            assert L.mi_blur_last_kernel().decode() == GENERIC, ((n, h, w, c), rx, ry)
            assert np.array_equal(got, ref_conv(img, **spec)), ((n, h, w, c), rx, ry)


def test_unaligned_pointers_take_the_generic_kernel(pkg, L, torch_cuda):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(2, 40, 64, 3), dtype=np.uint8)
    for (rx, ry, mode) in ((1, 1, "mag"), (3, 2, "sat"), (7, 7, "abs")):
        check_unaligned_pointers(CONV, pkg, L, torch_cuda, img, cr.make_kernel(pkg, **cr.random_kernel(rng, rx, ry, mode=mode)))


def test_bands_inside_the_image(pkg, L, torch_cuda):
    rng = np.random.default_rng(12)
    for (h, w, c) in ((64, 80, 3), (37, 17, 3), (90, 64, 4), (40, 48, 1)):
        img = rng.integers(0, 256, size=(1, h, w, c), dtype=np.uint8)
        for (rx, ry, mode) in ((1, 1, "mag"), (2, 2, "sat"), (3, 5, "abs"), (7, 7, "sat")):
            k = cr.make_kernel(pkg, **cr.random_kernel(rng, rx, ry, zeros=0.2, mode=mode))
            check_bands_inside_the_image(CONV, pkg, L, torch_cuda, img, k)


def test_batch_over_2gib(pkg, L, torch_cuda):
    """A batch of more than 2^31 bytes: 64-bit image offsets, the last image checked."""
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, size=(1, 1024, 1024, 3), dtype=np.uint8)
    n = 720                                                   # 2.26 GB in, as much out
    check_batch_over_2gib(CONV, pkg, L, torch_cuda, img, [cr.make_kernel(pkg, **SOBEL)], n, same=(0, n // 2, n - 2))


def test_refusals_and_empty_batch(pkg, L, torch_cuda):
    d = torch_cuda.zeros(4096, dtype=torch_cuda.uint8, device="cuda")
    p, q = d.data_ptr(), d.data_ptr() + 2048
    good = pkg.Conv.preset("sobel_mag")
    for field, v in (("rx", 8), ("ry", -1), ("mode", 3), ("shift", 17), ("bias", 2 ** 24 + 1)):
        bad = pkg.Conv.preset("sobel_mag")
        setattr(bad, field, v)
        assert L.mi_blur_enqueue_conv(p, q, 16, 8, 3, 1, C.byref(bad), None) == pkg.ERR_INVALID, field
        assert L.mi_blur_enqueue_conv_band(p, q, 16, 8, 3, 0, 8, C.byref(bad), None) == pkg.ERR_INVALID, field
    bad = pkg.Conv.preset("sobel_mag")
    bad.k2[4] = 32767
    bad.k2[5] = 32767                                            # sum |K2| = 65542
    assert L.mi_blur_enqueue_conv(p, q, 16, 8, 3, 1, C.byref(bad), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_conv(p, q, 16, 8, 3, 1, None, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_conv(p, p, 16, 8, 3, 1, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_conv(None, q, 16, 8, 3, 1, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_conv(p, q, 0, 8, 3, 1, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_conv(p, q, 16, 8, 3, -1, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_conv_band(p, q, 16, 8, 3, 6, 2, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_conv_band(p, q, 16, 8, 3, 0, 9, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_conv(p, q, 16, 8, 3, 0, C.byref(good), None) == pkg.OK
    torch_cuda.cuda.synchronize()


def test_saturation_and_floor_on_both_kernels(pkg, L, torch_cuda):
    for c, (h, w), kernel in ((1, (40, 64), TILED), (3, (33, 48), TILED), (1, (20, 31), GENERIC), (3, (17, 19), GENERIC)):
        for q, (img, spec) in enumerate(cr.saturation_cases(h, w, c)):
            got = gpu_run(CONV, pkg, L, torch_cuda, img, cr.make_kernel(pkg, **spec))
            assert L.mi_blur_last_kernel().decode() == kernel
            assert np.array_equal(got, ref_conv(img, **spec)), (c, kernel, q, spec["mode"], spec["shift"], spec["bias"])


def test_zero_padded_and_all_zero_kernels(pkg, L, torch_cuda):
    rng = np.random.default_rng(10)
    img = rng.integers(0, 256, size=(1, 40, 64, 3), dtype=np.uint8)
    spec = cr.random_kernel(rng, 2, 1, mode="mag")
    a = gpu_run(CONV, pkg, L, torch_cuda, img, cr.make_kernel(pkg, **spec))
    assert np.array_equal(a, ref_conv(img, **spec))
    for (rx, ry) in ((3, 1), (2, 4), (5, 6), (7, 7)):            # other column classes, more rows
        big = dict(spec)
        for t in ("K", "K2"):
            big[t] = np.zeros((2 * ry + 1, 2 * rx + 1), np.int64)
            big[t][ry - 1:ry + 2, rx - 2:rx + 3] = spec[t]
        assert np.array_equal(gpu_run(CONV, pkg, L, torch_cuda, img, cr.make_kernel(pkg, **big)), a), (rx, ry)
    Z = np.zeros((7, 9), np.int64)
    for shift, bias in ((0, 77), (0, 300), (0, -5), (4, 2047)):
        got = gpu_run(CONV, pkg, L, torch_cuda, img, cr.make_kernel(pkg, Z, shift, bias))
        assert (got == min(max(bias >> shift, 0), 255)).all()


def test_gpu_and_cpu_agree_on_the_synthetic_stream(pkg, L, torch_cuda):
    rng = np.random.default_rng(17)
    random_7x5 = cr.random_kernel(rng, 3, 2, mode="sat")         # 7 columns x 5 rows
    assert random_7x5["K"].shape == (5, 7)
    check_synthetic_stream(CONV, pkg, L, torch_cuda, (pkg.Conv.preset("sobel_mag"), pkg.Conv.preset("sharpen"), cr.make_kernel(pkg, **random_7x5)),
                           (200, 256, 256, 3), fill_threads=8, cpu_threads=16, check_kernel=True)


def test_context_with_a_conv(pkg, L, torch_cuda):
    """Every submit form of a GPU context takes the filter: pageable, pinned (one launch: not the batch server), strided
    bands, one band, planar."""
    rng = np.random.default_rng(21)
    n, h, w, c = 6, 240, 320, 3                                # 1.38 MB of output per submit: the server size class
    img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    for spec in (SOBEL, cr.random_kernel(rng, 3, 2, zeros=0.3, mode="sat"), cr.random_kernel(rng, 7, 7, mode="abs")):
        check_gpu_context(CONV, pkg, L, img, cr.make_kernel(pkg, **spec), pinned_repeats=2)


def test_python_functions(pkg, torch_cuda):
    rng = np.random.default_rng(30)
    imgs = rng.integers(0, 256, size=(4, 90, 128, 3), dtype=np.uint8)
    cpu = pkg.DEVICE_CPU
    assert np.array_equal(pkg.sobel(imgs), ref_conv(imgs, **SOBEL))
    for axis in ("x", "y", "mag"):
        assert np.array_equal(pkg.sobel(imgs, axis), pkg.sobel(imgs, axis, device=cpu)), axis
        assert np.array_equal(pkg.scharr(imgs, axis, batch=3), pkg.scharr(imgs, axis, device=cpu)), axis
    for conn in (4, 8):
        assert np.array_equal(pkg.laplacian(imgs, conn), pkg.laplacian(imgs, conn, device=cpu))
    assert np.array_equal(pkg.sharpen(imgs), ref_conv(imgs, **SHARPEN))
    spec = cr.random_kernel(rng, 5, 3, mode="mag")
    got = pkg.filter2d(imgs, spec["K"], spec["shift"], spec["bias"], "mag", spec["K2"])
    assert np.array_equal(got, ref_conv(imgs, **spec))
    assert np.array_equal(got, pkg.filter2d(imgs, spec["K"], spec["shift"], spec["bias"], "mag", spec["K2"], device=cpu))
    g = imgs[0, :, :, 0]
    got = pkg.sobel(g)
    assert got.shape == g.shape and np.array_equal(got, ref_conv(g[None, :, :, None], **SOBEL)[0, :, :, 0])


def test_hosts_conv_on_the_gpu(apps, torch_cuda, tmp_path):
    het, spl = apps
    rng = np.random.default_rng(40)
    img = rng.integers(0, 256, size=(240, 320, 3), dtype=np.uint8)
    write_ppm(tmp_path / "in.ppm", img)
    emboss = dict(K=[[-2, -1, 0], [-1, 1, 1], [0, 1, 2]], bias=128)
    for name, spec in (("sobel", SOBEL), ("emboss", emboss)):
        want = ref_conv(img[None], **spec)[0]
        for mode in ("gpu", "both"):
            out = f"{mode}_{name}.ppm"
            r = subprocess.run([het, mode, "0.7", "35", "--image", "in.ppm", "--images", "100", "--conv", name, "--save", out],
                               cwd=tmp_path, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout + r.stderr
            assert f"Blur kernel: 3x3 convolution ({name})\n" in r.stdout
            assert np.array_equal(read_ppm(tmp_path / out), want), (mode, name)
    r = subprocess.run([spl, "0.6", "16", "--image", "in.ppm", "--images", "48", "--conv", "sharpen", "--save", "s.ppm"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Halo size: 1 row(s)" in r.stdout and "Blur kernel: 3x3 convolution (sharpen)\n" in r.stdout
    assert np.array_equal(read_ppm(tmp_path / "s.ppm"), ref_conv(img[None], **SHARPEN)[0])
