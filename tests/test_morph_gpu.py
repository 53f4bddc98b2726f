"""Erode / dilate / morphological gradient on a real MI355X (-m gpu): mi_blur_enqueue_morph / _band, a context given the
filter by mi_blur_ctx_set_morph, erode() / dilate() / morph_gradient() and the hosts' flags, byte for byte against a numpy
restatement of the definition in include/mi_blur.h (morph_ref.py) and against the CPU device.

Inputs as in tests/test_morph_host.py: sparse impulses (more than 33 apart, one channel each, on the image's edges and on
both sides of every tile seam of blur_morph_tiled_kernel and of the slots a wave stages), ramps, checkerboards and
low-amplitude noise at every radius; random bytes at the small radii only."""
import subprocess

import numpy as np
import pytest

from filter_harness import (MORPH, apps, check_batch_over_2gib, check_bands_inside_the_image, check_gpu_context,  # noqa: F401
                            check_synthetic_stream, check_unaligned_pointers, gpu_run, read_ppm, torch_cuda, write_ppm)
from morph_ref import (DILATE, ERODE, GRADIENT, OPS, TILE_CHUNKS, TILE_ROWS, _finish, impulse_batch, mixed, ref_lo_hi, ref_morph,
                       ref_morph_2d, seam_impulses, structured)

pytestmark = pytest.mark.gpu

TILED, GENERIC = MORPH.fast, MORPH.generic


def test_separable_restatement_is_the_2d_definition():
    rng = np.random.default_rng(0)
    for (n, h, w, c) in ((2, 9, 13, 3), (1, 40, 37, 1)):
        for img in [impulse_batch(h, w, c, [(0, 0), (h - 1, w - 1), (h // 2, w // 3)])] + structured(rng, n, h, w, c):
            for rx in (0, 1, 2, 5, 16):
                for ry in (0, 1, 2, 5, 16):
                    for op in OPS:
                        assert np.array_equal(ref_morph(img, op, rx, ry), ref_morph_2d(img, op, rx, ry)), ((n, h, w, c), op, rx, ry)


# rows of whole 16-byte chunks with 1-4 channels (the tiled kernel at every radius) and everything else
ALIGNED = [(2, 64, 80, 3), (1, 40, 64, 4), (3, 33, 16, 1), (1, 100, 1024, 1), (1, 37, 2000, 4), (2, 70, 96, 2),
           (1, 1, 16, 1), (1, 2, 48, 1), (1, 300, 512, 3), (1, 5, 32, 2)]
RAGGED = [(1, 17, 33, 3), (2, 30, 250, 3), (1, 9, 5, 1), (1, 31, 29, 2), (1, 50, 7, 5), (1, 24, 64, 5), (1, 1, 1, 3),
          (1, 12, 16, 6), (1, 10, 20, 7), (1, 14, 18, 8)]
PAIRS = [(0, 0), (1, 1), (2, 2), (3, 0), (0, 3), (4, 5), (7, 8), (9, 3), (5, 12), (16, 15), (13, 16), (16, 16)]


def test_enqueue_morph_matches_numpy(pkg, L, torch_cuda):
    rng = np.random.default_rng(2024)
    for shapes, kern in ((ALIGNED, TILED), (RAGGED, GENERIC)):
        for (n, h, w, c) in shapes:
            imgs = [seam_impulses(h, w, c, 16, 16), mixed(rng, n, h, w, c)]
            rnd = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
            for rx, ry in PAIRS:
                for k, img in enumerate(imgs + ([rnd] if max(rx, ry) <= 2 else [])):
                    lo, hi = ref_lo_hi(img, rx, ry)
                    for op in OPS:
                        got = gpu_run(MORPH, pkg, L, torch_cuda, img, (op, rx, ry))
                        assert L.mi_blur_last_kernel().decode() == kern, ((n, h, w, c), op, rx, ry)
                        assert np.array_equal(got, _finish(lo, hi, op)), ((n, h, w, c), op, rx, ry, k)


def test_every_radius_on_impulses(pkg, L, torch_cuda):
    """rx and ry each through 0..16 (the other at a fixed value): exact rectangles around impulses at seams and edges."""
    rng = np.random.default_rng(7)
    for (h, w, c) in ((70, 688, 3), (66, 1040, 1), (40, 272, 4), (35, 528, 2)):
        noise = rng.integers(100, 141, size=(1, h, w, c), dtype=np.uint8)
        for r in range(17):
            for rx, ry in ((r, 2), (3, r), (r, r)):
                img = np.concatenate([seam_impulses(h, w, c, rx, ry), noise])
                lo, hi = ref_lo_hi(img, rx, ry)
                for op in OPS:
                    got = gpu_run(MORPH, pkg, L, torch_cuda, img, (op, rx, ry))
                    assert L.mi_blur_last_kernel().decode() == TILED
                    assert np.array_equal(got, _finish(lo, hi, op)), ((h, w, c), op, rx, ry)


def test_tile_edges(pkg, L, torch_cuda):
    """Heights and widths around the tile's row and chunk-column counts (one less, equal, one more, two tiles plus one),
    at radii on both sides of every power of two up to 16."""
    rng = np.random.default_rng(8)
    radii = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16)
    for c in (1, 3):
        for k, h in enumerate((TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, 2 * TILE_ROWS + 1)):
            for j, chunks in enumerate((TILE_CHUNKS - 1, TILE_CHUNKS, TILE_CHUNKS + 1, 2 * TILE_CHUNKS + 1)):
                cpr = chunks * c                                 # rows of whole chunks whatever the channel count
                w = cpr * 16 // c
                img = np.concatenate([seam_impulses(h, w, c, 16, 16), mixed(rng, 1, h, w, c)])
                for i, r in enumerate(radii):
                    rx, ry = (r, radii[(i + 3) % len(radii)]) if (k + j) % 2 else (r, r)
                    op = OPS[(i + k + j) % 3]
                    got = gpu_run(MORPH, pkg, L, torch_cuda, img, (op, rx, ry))
                    assert L.mi_blur_last_kernel().decode() == TILED
                    assert np.array_equal(got, ref_morph(img, op, rx, ry)), ((h, w, c), op, rx, ry)


def test_enqueue_morph_unaligned_pointers(pkg, L, torch_cuda):
    rng = np.random.default_rng(5)
    img = mixed(rng, 2, 40, 64, 3)
    for filt in ((ERODE, 1, 1), (DILATE, 6, 2), (GRADIENT, 16, 9)):
        check_unaligned_pointers(MORPH, pkg, L, torch_cuda, img, filt)


def test_bands_inside_the_image(pkg, L, torch_cuda):
    rng = np.random.default_rng(12)
    for (h, w, c) in ((64, 80, 3), (37, 17, 3), (90, 64, 4), (40, 48, 1)):
        img = mixed(rng, 1, h, w, c)
        for filt in ((ERODE, 1, 1), (DILATE, 2, 4), (GRADIENT, 7, 2), (ERODE, 3, 16), (DILATE, 16, 0)):
            check_bands_inside_the_image(MORPH, pkg, L, torch_cuda, img, filt, skip_empty=True)


def test_enqueue_morph_refusals(pkg, L, torch_cuda):
    d = torch_cuda.zeros(4096, dtype=torch_cuda.uint8, device="cuda")
    p, q = d.data_ptr(), d.data_ptr() + 2048
    for op in (-1, 3):
        assert L.mi_blur_enqueue_morph(p, q, 16, 8, 3, op, 1, 1, 1, None) == pkg.ERR_INVALID
    for rx, ry in ((-1, 0), (0, -1), (17, 0), (0, 17)):
        assert L.mi_blur_enqueue_morph(p, q, 16, 8, 3, ERODE, rx, ry, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph(p, p, 16, 8, 3, ERODE, 1, 1, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph(None, q, 16, 8, 3, ERODE, 1, 1, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph(p, q, 0, 8, 3, ERODE, 1, 1, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph(p, q, 16, 8, 3, ERODE, 1, 1, -1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph_band(p, q, 16, 8, 3, DILATE, 1, 1, 6, 2, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph_band(p, q, 16, 8, 3, DILATE, 1, 1, 0, 9, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph(p, q, 16, 8, 3, GRADIENT, 16, 16, 0, None) == pkg.OK


def test_batch_over_2gib(pkg, L, torch_cuda):
    """A batch of more than 2^31 bytes: 64-bit image offsets, the last image checked."""
    rng = np.random.default_rng(8)
    img = mixed(rng, 1, 1024, 1024, 3)
    n = 720                                                   # 2.26 GB in, as much out
    check_batch_over_2gib(MORPH, pkg, L, torch_cuda, img, ((ERODE, 2, 2), (GRADIENT, 9, 5)), n, same=(0, n // 2, n - 2))


def test_gpu_and_cpu_agree_on_the_synthetic_stream(pkg, L, torch_cuda):
    check_synthetic_stream(MORPH, pkg, L, torch_cuda, [(op, r, r) for op in OPS for r in (1, 4, 16)], (1000, 256, 256, 3),
                           fill_threads=8, cpu_threads=16)


def test_context_with_a_morph(pkg, L, torch_cuda):
    """Every submit form of a GPU context takes the filter: pageable, pinned (one launch: not the batch server), strided
    bands, one band, planar."""
    rng = np.random.default_rng(21)
    img = mixed(rng, 6, 240, 320, 3)                           # 1.38 MB of output per submit: the server size class
    for filt in ((ERODE, 1, 1), (DILATE, 4, 2), (GRADIENT, 16, 16)):
        check_gpu_context(MORPH, pkg, L, img, filt, pinned_repeats=2)


def test_morphology_functions_python(pkg, torch_cuda):
    rng = np.random.default_rng(30)
    imgs = mixed(rng, 4, 90, 128, 3)
    for fn, op in ((pkg.erode, ERODE), (pkg.dilate, DILATE), (pkg.morph_gradient, GRADIENT)):
        for k in (1, 3, 7, 17, 33):
            assert np.array_equal(fn(imgs, k), ref_morph(imgs, op, k // 2, k // 2)), (op, k)
        assert np.array_equal(fn(imgs, (9, 3), batch=3), ref_morph(imgs, op, 4, 1)), op
        g = imgs[0, :, :, 0]
        assert np.array_equal(fn(g, (5, 21)), ref_morph(g[None, :, :, None], op, 2, 10)[0, :, :, 0])


def test_hosts_morph_on_the_gpu(apps, torch_cuda, tmp_path):
    het, spl = apps
    rng = np.random.default_rng(40)
    img = mixed(rng, 1, 240, 320, 3)[0]
    write_ppm(tmp_path / "in.ppm", img)
    for flag, k, op, name in (("--erode", 5, ERODE, "erode"), ("--dilate", 7, DILATE, "dilate"),
                              ("--morph-gradient", 33, GRADIENT, "morphological gradient")):
        want = ref_morph(img[None], op, k // 2, k // 2)[0]
        for mode in ("gpu", "both"):
            out = f"{mode}{k}.ppm"
            r = subprocess.run([het, mode, "0.7", "35", "--image", "in.ppm", "--images", "100", flag, str(k), "--save", out],
                               cwd=tmp_path, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout + r.stderr
            assert f"Blur kernel: {k}x{k} {name}\n" in r.stdout
            assert np.array_equal(read_ppm(tmp_path / out), want), (mode, flag)
    r = subprocess.run([spl, "0.6", "16", "--image", "in.ppm", "--images", "48", "--dilate", "7", "--save", "s.ppm"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Halo size: 3 row(s)" in r.stdout and "Blur kernel: 7x7 dilate\n" in r.stdout
    assert np.array_equal(read_ppm(tmp_path / "s.ppm"), ref_morph(img[None], DILATE, 3, 3)[0])
