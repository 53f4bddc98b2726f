"""Bilateral filter on a real MI355X (-m gpu): mi_blur_enqueue_bilateral / _band, a context given the filter by
mi_blur_ctx_set_bilateral, bilateral_filter() and the hosts' --bilateral, byte for byte against the numpy restatement of
the definition in include/mi_blur.h (bilateral_ref.py) and against the CPU device.  0x5A guard bytes surround every output."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import bilateral_ref as br
from bilateral_ref import ref_bilateral
from filter_harness import (BILATERAL, TILE_CHUNKS, TILE_ROWS, apps, check_batch_over_2gib, check_bands_inside_the_image,  # noqa: F401
                            check_gpu_context, check_synthetic_stream, check_unaligned_pointers, cpu_run, gpu_run, read_ppm,
                            seam_image, torch_cuda, write_ppm)

pytestmark = pytest.mark.gpu

TILED, GENERIC = BILATERAL.fast, BILATERAL.generic
RADII = tuple(range(1, 9))

# rows of whole 16-byte chunks with 1-4 channels (the tiled kernel at every radius) and everything else
ALIGNED = {1: (2, 70, 1040), 2: (1, 65, 536), 3: (2, 66, 688), 4: (1, 40, 272)}        # c -> (n, h, w): several tiles both ways
RAGGED = [(1, 17, 33, 3), (2, 30, 250, 3), (1, 9, 5, 1), (1, 31, 29, 2), (1, 50, 7, 5), (1, 24, 64, 5), (1, 1, 1, 3), (1, 12, 16, 6), (1, 3, 15, 1)]


def test_tiled_kernel_every_radius_and_channel_count(pkg, L, torch_cuda):
    rng = np.random.default_rng(2024)
    for c, (n, h, w) in ALIGNED.items():
        imgs = [rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8), seam_image(rng, h, w, c)]
        for r in RADII:
            for t, tables in enumerate((br.gauss_tables(0, 25.0, r), br.random_tables(rng, r, zeros=0.3))):
                k = br.make_kernel(pkg, *tables)
                for q, img in enumerate(imgs):
                    got = gpu_run(BILATERAL, pkg, L, torch_cuda, img, k)
                    assert L.mi_blur_last_kernel().decode() == TILED, (c, r)
                    assert np.array_equal(got, ref_bilateral(img, *tables)), (c, r, t, q)
                    assert np.array_equal(got, cpu_run(BILATERAL, pkg, L, img, k, 8, prefill=False)), (c, r, t, q)


def test_tile_edges(pkg, L, torch_cuda):
    """Heights and widths around the tile's row and chunk-column counts (one less, equal, one more, two tiles plus one)."""
    rng = np.random.default_rng(8)
    for c in (1, 3):
        for a, h in enumerate((TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, 2 * TILE_ROWS + 1)):
            for b, chunks in enumerate((TILE_CHUNKS - 1, TILE_CHUNKS, TILE_CHUNKS + 1, 2 * TILE_CHUNKS + 1)):
                w = chunks * 16                                  # cpr = chunks * c: rows of whole chunks whatever the channel count
                img = seam_image(rng, h, w, c)
                for r in ((1, 4, 8), (2, 5), (3, 6), (7,))[(a + b) % 4]:
                    tables = br.random_tables(rng, r, zeros=0.2)
                    got = gpu_run(BILATERAL, pkg, L, torch_cuda, img, br.make_kernel(pkg, *tables))
                    assert L.mi_blur_last_kernel().decode() == TILED
                    assert np.array_equal(got, ref_bilateral(img, *tables)), (h, w, c, r)


def test_input_kinds(pkg, L, torch_cuda):
    rng = np.random.default_rng(3)
    for (n, h, w, c) in ((1, 50, 96, 3), (2, 37, 64, 1)):
        for q, img in enumerate(br.input_kinds(rng, n, h, w, c)):
            for r in (1, 2, 4, 8):
                for tables in (br.gauss_tables(0, 12.0, r), br.random_tables(rng, r)):
                    got = gpu_run(BILATERAL, pkg, L, torch_cuda, img, br.make_kernel(pkg, *tables))
                    assert L.mi_blur_last_kernel().decode() == TILED
                    assert np.array_equal(got, ref_bilateral(img, *tables)), ((n, h, w, c), q, r)


def test_generic_kernel(pkg, L, torch_cuda):
    rng = np.random.default_rng(4)
    for (n, h, w, c) in RAGGED:
        img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
        for r in RADII:
            tables = br.random_tables(rng, r, zeros=0.3) if r % 2 else br.gauss_tables(0, 30.0, r)
            got = gpu_run(BILATERAL, pkg, L, torch_cuda, img, br.make_kernel(pkg, *tables))
            assert L.mi_blur_last_kernel().decode() == GENERIC, ((n, h, w, c), r)
            assert np.array_equal(got, ref_bilateral(img, *tables)), ((n, h, w, c), r)


def test_unaligned_pointers_take_the_generic_kernel(pkg, L, torch_cuda):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(2, 40, 64, 3), dtype=np.uint8)
    for r in (1, 3, 8):
        check_unaligned_pointers(BILATERAL, pkg, L, torch_cuda, img, br.make_kernel(pkg, *br.random_tables(rng, r)))


def test_bands_inside_the_image(pkg, L, torch_cuda):
    rng = np.random.default_rng(12)
    for (h, w, c) in ((64, 80, 3), (37, 17, 3), (90, 64, 4), (40, 48, 1)):
        img = rng.integers(0, 256, size=(1, h, w, c), dtype=np.uint8)
        for r in (1, 2, 5, 8):
            k = br.make_kernel(pkg, *br.random_tables(rng, r, zeros=0.2))
            check_bands_inside_the_image(BILATERAL, pkg, L, torch_cuda, img, k)


def test_batch_over_2gib(pkg, L, torch_cuda):
    """A batch of more than 2^31 bytes: 64-bit image offsets, the last image checked."""
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, size=(1, 1024, 1024, 3), dtype=np.uint8)
    n = 720                                                   # 2.26 GB in, as much out
    k = br.make_kernel(pkg, *br.gauss_tables(0, 25.0, 1))
    check_batch_over_2gib(BILATERAL, pkg, L, torch_cuda, img, [k], n, same=(0, n // 2, n - 2))


def test_refusals_and_empty_batch(pkg, L, torch_cuda):
    d = torch_cuda.zeros(4096, dtype=torch_cuda.uint8, device="cuda")
    p, q = d.data_ptr(), d.data_ptr() + 2048
    good = pkg.Bilateral.gauss(0.0, 25.0, 2)
    bad = pkg.Bilateral.gauss(0.0, 25.0, 2)
    bad.radius = 9
    assert L.mi_blur_enqueue_bilateral(p, q, 16, 8, 3, 1, C.byref(bad), None) == pkg.ERR_INVALID
    bad.radius, bad.range[0] = 2, 0
    assert L.mi_blur_enqueue_bilateral(p, q, 16, 8, 3, 1, C.byref(bad), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_bilateral(p, q, 16, 8, 3, 1, None, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_bilateral(p, p, 16, 8, 3, 1, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_bilateral(None, q, 16, 8, 3, 1, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_bilateral(p, q, 0, 8, 3, 1, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_bilateral(p, q, 16, 8, 3, -1, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_bilateral_band(p, q, 16, 8, 3, 6, 2, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_bilateral_band(p, q, 16, 8, 3, 0, 9, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_bilateral(p, q, 16, 8, 3, 0, C.byref(good), None) == pkg.OK
    torch_cuda.cuda.synchronize()


def test_division_boundaries(pkg, L, torch_cuda):
    """Two-valued windows whose counts step through every split, S all 1 and R all 255: quotients on and beside .5; then
    random tables on the same images and on random bytes, where num / den is arbitrary."""
    rng = np.random.default_rng(6)
    ones = np.full(256, 255, np.int64)
    for (h, w, c) in ((64, 128, 1), (40, 80, 2)):
        img = br.division_images(h, w, c)
        for r in RADII:
            S = np.ones((2 * r + 1, 2 * r + 1), np.int64)
            for tables in ((S, ones), (S * 3, ones // 5), br.random_tables(rng, r)):
                got = gpu_run(BILATERAL, pkg, L, torch_cuda, img, br.make_kernel(pkg, *tables))
                assert L.mi_blur_last_kernel().decode() == TILED
                assert np.array_equal(got, ref_bilateral(img, *tables)), (h, w, c, r)
    # the largest sums the validation admits
    S = np.full((17, 17), 226, np.int64)
    S.reshape(-1)[:65535 - 226 * 289] += 1
    for img in (np.full((1, 40, 64, 1), 255, np.uint8), rng.integers(200, 256, size=(1, 40, 64, 1), dtype=np.uint8),
                rng.integers(0, 256, size=(1, 40, 64, 1), dtype=np.uint8)):
        got = gpu_run(BILATERAL, pkg, L, torch_cuda, img, br.make_kernel(pkg, S, ones))
        assert np.array_equal(got, ref_bilateral(img, S, ones))
        got = gpu_run(BILATERAL, pkg, L, torch_cuda, img[:, :, :63], br.make_kernel(pkg, S, ones))       # the generic kernel's division
        assert L.mi_blur_last_kernel().decode() == GENERIC
        assert np.array_equal(got, ref_bilateral(img[:, :, :63], S, ones))


def test_gpu_and_cpu_agree_on_the_synthetic_stream(pkg, L, torch_cuda):
    check_synthetic_stream(BILATERAL, pkg, L, torch_cuda, [pkg.Bilateral.gauss(0.0, 25.0, r) for r in (1, 2, 4)], (200, 256, 256, 3),
                           fill_threads=8, cpu_threads=16)


def test_context_with_a_bilateral(pkg, L, torch_cuda):
    """Every submit form of a GPU context takes the filter: pageable, pinned (one launch: not the batch server), strided
    bands, one band, planar."""
    rng = np.random.default_rng(21)
    n, h, w, c = 6, 240, 320, 3                                # 1.38 MB of output per submit: the server size class
    img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    for tables in (br.gauss_tables(0, 25.0, 1), br.random_tables(rng, 3, zeros=0.3), br.gauss_tables(0, 40.0, 8)):
        check_gpu_context(BILATERAL, pkg, L, img, br.make_kernel(pkg, *tables), pinned_repeats=2)


def test_bilateral_filter_python(pkg, torch_cuda):
    rng = np.random.default_rng(30)
    imgs = rng.integers(0, 256, size=(4, 90, 128, 3), dtype=np.uint8)
    for k in (3, 5, 9, 17):
        assert np.array_equal(pkg.bilateral_filter(imgs, k), ref_bilateral(imgs, *br.gauss_tables(k / 4.0, 25.0, k // 2))), k
    assert np.array_equal(pkg.bilateral_filter(imgs, 7, sigma_color=50.0, sigma_space=3.0, batch=3), ref_bilateral(imgs, *br.gauss_tables(3.0, 50.0, 3)))
    g = imgs[0, :, :, 0]
    assert np.array_equal(pkg.bilateral_filter(g, 5), ref_bilateral(g[None, :, :, None], *br.gauss_tables(1.25, 25.0, 2))[0, :, :, 0])
    assert np.array_equal(pkg.bilateral_filter(imgs, 5), pkg.bilateral_filter(imgs, 5, device=pkg.DEVICE_CPU))


def test_hosts_bilateral_on_the_gpu(apps, torch_cuda, tmp_path):
    het, spl = apps
    rng = np.random.default_rng(40)
    img = rng.integers(0, 256, size=(240, 320, 3), dtype=np.uint8)
    write_ppm(tmp_path / "in.ppm", img)
    for k, extra, sc, ss in ((5, [], 25.0, 1.25), (17, ["--sigma-color", "40", "--sigma-space", "5"], 40.0, 5.0)):
        want = ref_bilateral(img[None], *br.gauss_tables(ss, sc, k // 2))[0]
        for mode in ("gpu", "both"):
            out = f"{mode}{k}.ppm"
            r = subprocess.run([het, mode, "0.7", "35", "--image", "in.ppm", "--images", "100", "--bilateral", str(k)] + extra +
                               ["--save", out], cwd=tmp_path, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout + r.stderr
            assert f"Blur kernel: {k}x{k} bilateral (sigma_color {sc:g}, sigma_space {ss:g})\n" in r.stdout
            assert np.array_equal(read_ppm(tmp_path / out), want), (mode, k)
    r = subprocess.run([spl, "0.6", "16", "--image", "in.ppm", "--images", "48", "--bilateral", "7", "--save", "s.ppm"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Halo size: 3 row(s)" in r.stdout and "Blur kernel: 7x7 bilateral (sigma_color 25, sigma_space 1.75)\n" in r.stdout
    assert np.array_equal(read_ppm(tmp_path / "s.ppm"), ref_bilateral(img[None], *br.gauss_tables(1.75, 25.0, 3))[0])
