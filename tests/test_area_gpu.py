"""The area resize on the GPU (mi_blur_enqueue_area, mi_blur_ctx_set_area, area_resize(), the hosts' --resize WxH --area):
exact bytes against the numpy restatement of the header's definition (area_ref.py), and which of the two kernels took
each launch."""
import subprocess

import numpy as np
import pytest

from area_ref import AREA, TILE_ROWS, blocks, ref_area, ref_axis, takes_tiled, tile_geometry
from resample_harness import (apps, check_gpu_context, check_pointer_offsets, check_synthetic_stream, gpu_run, last, read_ppm, torch_cuda,  # noqa: F401
                              write_ppm)

pytestmark = pytest.mark.gpu

TILED, GENERIC = AREA.tiled, AREA.generic
CHANNELS = (1, 2, 3, 4)


def unit(c):
    """Chunks of the smallest run that starts and ends on a pixel."""
    return 3 if c == 3 else 1


def width(c, units):
    """Pixels of a row of `units` units of c channels."""
    return units * unit(c) * 16 // c


# (H, input units, Ho, output units): / 2, / 3, / 4, 64 -> 63 rows over 8 -> 7 units, 100 -> 37 rows over 7 -> 3 units, x only,
# y only, equal size, one output row, the cap on rows (1024 -> 16), the cap on columns (64 units -> 1: one chunk, or one
# 3-chunk unit under 192 input chunks), / 32 and a ratio of 50 x 43.3 (3 channels: row groups of 128 and 256 threads)
RATIOS = [(18, 12, 9, 6), (21, 12, 7, 4), (24, 16, 6, 4), (64, 8, 63, 7), (100, 7, 37, 3), (11, 10, 11, 3), (30, 5, 7, 5), (13, 5, 13, 5), (40, 6, 1, 4),
          (1024, 2, 16, 1), (3, 64, 2, 1), (64, 32, 5, 1), (130, 50, 3, 1)]


def run_tiled(pkg, L, torch, img, wo, ho):
    assert takes_tiled(img.shape, wo, ho)
    got = gpu_run(AREA, pkg, L, torch, img, (wo, ho))
    assert last(L) == TILED
    return got


@pytest.mark.parametrize("c", CHANNELS)
def test_aligned_reductions_take_the_tiled_kernel(pkg, L, torch_cuda, c):
    rng = np.random.default_rng(40 + c)
    groups = set()
    for h, iu, ho, ou in RATIOS:
        w, wo = width(c, iu), width(c, ou)
        img = rng.integers(0, 256, size=(2, h, w, c), dtype=np.uint8)
        got = run_tiled(pkg, L, torch_cuda, img, wo, ho)
        assert np.array_equal(got, ref_area(img, wo, ho)), (h, w, c, wo, ho)
        if (wo, ho) == (w, h):
            assert np.array_equal(got, img)                              # same size: the identity, through the tiled kernel
        groups.add(tile_geometry(w, wo, ho, c)[3])
    assert groups == ({64, 128, 256} if c == 3 else {64})                # every size of row group the kernel has


@pytest.mark.parametrize("c", CHANNELS)
def test_tile_rows_and_strip_widths(pkg, L, torch_cuda, c):
    """Output rows one below, at and one above the tile's rows, and at / 2 an output row one unit below, at and one unit
    above the widest single strip: one strip, one strip, more than one strip."""
    rng = np.random.default_rng(50 + c)
    m = (64 - 3) // (2 * unit(c))                                        # units of the widest strip at / 2 (tile_geometry)
    for ho in (TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, 2 * TILE_ROWS + 1):
        for k in (-1, 0, 1):
            wo, w = width(c, m + k), width(c, 2 * (m + k))
            ncols, cpr, rows, group = tile_geometry(w, wo, ho, c)
            assert rows == TILE_ROWS and group == 64 and (-(-cpr // ncols) > 1) == (k == 1) and (k == 1 or ncols == cpr == (m + k) * unit(c))
            img = rng.integers(0, 256, size=(1, 2 * ho + (ho % 2), w, c), dtype=np.uint8)     # an odd row count in every other case
            assert np.array_equal(run_tiled(pkg, L, torch_cuda, img, wo, ho), ref_area(img, wo, ho)), (ho, k)


def test_batches_either_side_of_the_xcd_remap(pkg, L, torch_cuda):
    """Grids of 15 and of 18 workgroups: below 16 the blocks take the tiles in order, from 16 on through the XCD remap."""
    h, w, c, wo, ho = 24, 96, 3, 48, 10
    assert blocks(1, w, wo, ho, c) == 3
    rng = np.random.default_rng(60)
    for n in (5, 6, 11):
        img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
        assert (blocks(n, w, wo, ho, c) >= 16) == (n >= 6)
        assert np.array_equal(run_tiled(pkg, L, torch_cuda, img, wo, ho), ref_area(img, wo, ho)), n


def test_totals_are_64_bit(pkg, L, torch_cuda):
    """8192 x 4096 x 1 of 255 -> 128 x 64 (the cap on both axes): S = 255 * 2^25, so a 32-bit total anywhere shows."""
    img = np.full((1, 4096, 8192, 1), 255, np.uint8)
    assert (run_tiled(pkg, L, torch_cuda, img, 128, 64) == 255).all()
    img[0, ::2] = 0                                                      # 127.5 rounds half up
    assert (run_tiled(pkg, L, torch_cuda, img, 128, 64) == 128).all()


def seam_images(rng, h, w, c, wo, ho):
    """Low-amplitude noise with 0 / 255 impulses (one channel each) and 0 / 255 step edges at the input pixels under every
    seam between output tiles (the last tap of the output row or column before it, the first tap of the one after) and on
    the borders; an all-255 image; impulses in the four corners."""
    ncols, cpr, trows, _ = tile_geometry(w, wo, ho, c)
    x_lo, x_hi, _, _ = ref_axis(w, wo)
    y_lo, y_hi, _, _ = ref_axis(h, ho)
    ocols = [s * 16 // c for s in range(ncols, cpr, ncols)]              # the first output pixel of every strip but the first
    rows = sorted({0, h - 1} | {int(v) for s in range(trows, ho, trows) for v in (y_hi[s - 1], y_lo[s])})
    cols = sorted({0, w - 1} | {int(v) for x in ocols for v in (x_hi[x - 1], x_lo[x])})
    img = rng.integers(118, 139, size=(4, h, w, c), dtype=np.uint8)
    k = 0
    for y in rows:
        for x in cols:
            img[0, y, x, k % c] = 255 if k % 2 else 0
            k += 1
    for s in rows[1:-1:2]:
        img[1, s:, : w // 2] = 255
        img[1, :s, w // 2:] = 0
    for s in cols[1:-1:2]:
        img[1, : h // 3, s:] = 255 - img[1, : h // 3, s:]
    img[2] = 255
    img[3] = 0
    for y in (0, h - 1):
        for x in (0, w - 1):
            img[3, y, x] = 255
    return img


@pytest.mark.parametrize("case", [(26, 1024, 1, 512, 13), (27, 768, 3, 256, 9), (50, 640, 2, 232, 19), (23, 512, 4, 300, 10), (70, 1040, 1, 384, 27)],
                         ids=lambda c: "x".join(map(str, c[:3])) + f"-{c[3]}x{c[4]}")
def test_tile_seams(pkg, L, torch_cuda, case):
    h, w, c, wo, ho = case
    ncols, cpr, trows, _ = tile_geometry(w, wo, ho, c)
    assert ho > trows and cpr > ncols                                    # more than one tile both ways
    img = seam_images(np.random.default_rng(7), h, w, c, wo, ho)
    got = run_tiled(pkg, L, torch_cuda, img, wo, ho)
    assert (got[2] == 255).all(), case
    assert np.array_equal(got, ref_area(img, wo, ho)), case


def test_other_launches_take_the_generic_kernel(pkg, L, torch_cuda):
    """5 channels, odd widths, enlargements, enlarge x with reduce y (and the reverse), 64 x 64 -> 1 x 1."""
    rng = np.random.default_rng(3)
    cases = [((1, 24, 64, 5), 32, 12), ((1, 50, 7, 5), 3, 20), ((1, 17, 33, 3), 16, 9), ((1, 17, 32, 3), 15, 9), ((2, 9, 5, 1), 11, 17),
             ((1, 16, 32, 1), 64, 32), ((1, 16, 32, 2), 96, 48), ((1, 40, 32, 1), 64, 10), ((1, 10, 64, 1), 32, 40), ((1, 1, 1, 3), 9, 9),
             ((1, 64, 64, 1), 1, 1), ((3, 64, 64, 4), 1, 1), ((1, 33, 47, 3), 47, 33)]
    for shape, wo, ho in cases:
        img = rng.integers(0, 256, size=shape, dtype=np.uint8)
        assert not takes_tiled(shape, wo, ho)
        got = gpu_run(AREA, pkg, L, torch_cuda, img, (wo, ho))
        assert last(L) == GENERIC, (shape, wo, ho)
        assert np.array_equal(got, ref_area(img, wo, ho)), (shape, wo, ho)
    img = rng.integers(0, 256, size=(1, 16, 32, 1), dtype=np.uint8)
    for k in (2, 3):                                                     # an integer enlargement replicates pixels
        assert np.array_equal(gpu_run(AREA, pkg, L, torch_cuda, img, (32 * k, 16 * k)), np.repeat(np.repeat(img, k, axis=1), k, axis=2))
    img = rng.integers(0, 256, size=(2, 35, 96, 2), dtype=np.uint8)      # aligned shape, pointers off 16 bytes
    check_pointer_offsets(AREA, pkg, L, torch_cuda, img, (40, 14))


def test_gpu_equals_cpu_device_on_the_synthetic_stream(pkg, L, torch_cuda):
    check_synthetic_stream(AREA, pkg, L, torch_cuda, [(160, 120), (112, 75), (107, 80), (320, 240), (640, 480), (5, 4), (400, 100)])


@pytest.mark.parametrize("target", [(80, 60), (100, 75)], ids=lambda t: "x".join(map(str, t)))
def test_gpu_context(pkg, L, torch_cuda, target):
    shape = (6, 120, 160, 3)
    img = np.random.default_rng(13).integers(0, 256, size=shape, dtype=np.uint8)
    kernel = TILED if takes_tiled(shape, *target) else GENERIC
    assert (kernel == TILED) == (target == (80, 60))
    check_gpu_context(AREA, pkg, L, img, target, kernel)


def test_numpy_function_on_the_gpu(pkg, L, torch_cuda):
    rng = np.random.default_rng(17)
    stack = rng.integers(0, 256, size=(3, 90, 128, 3), dtype=np.uint8)
    assert np.array_equal(pkg.area_resize(stack, (64, 45)), ref_area(stack, 64, 45))
    assert np.array_equal(pkg.area_resize(stack, (50, 31), batch=2), ref_area(stack, 50, 31))
    assert np.array_equal(pkg.area_resize(stack[0], (200, 61), batch=1), ref_area(stack[:1], 200, 61)[0])
    odd = rng.integers(0, 256, size=(45, 71), dtype=np.uint8)
    assert np.array_equal(pkg.area_resize(odd, (30, 20)), ref_area(odd[None, :, :, None], 30, 20)[0, :, :, 0])
    even = rng.integers(0, 256, size=(45, 64), dtype=np.uint8)
    assert np.array_equal(pkg.area_resize(even, (32, 20)), ref_area(even[None, :, :, None], 32, 20)[0, :, :, 0])


def test_hosts_area(pkg, apps, torch_cuda, tmp_path):
    het, split = apps
    rng = np.random.default_rng(19)
    img = rng.integers(0, 256, size=(240, 320, 3), dtype=np.uint8)
    src = tmp_path / "in.ppm"
    write_ppm(src, img)
    for size in ((160, 120), (100, 75)):
        want = ref_area(img[None], *size)[0]
        for run in (["gpu", "1.0", "35"], ["both", "0.7", "35"], ["cpu", "0", "35"]):
            dst = tmp_path / f"{run[0]}_{size[0]}.ppm"
            r = subprocess.run([het, *run, "--image", str(src), "--images", "100", "--resize", f"{size[0]}x{size[1]}", "--area", "--save", str(dst)],
                               capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            assert f"Blur kernel: area resize, 320x240 -> {size[0]}x{size[1]}" in r.stdout
            got = read_ppm(dst)
            assert got.shape == (size[1], size[0], 3) and np.array_equal(got, want), (run, size)
    r = subprocess.run([het, "gpu", "1.0", "35", "--image", str(src), "--images", "10", "--resize", "160x120", "--area", "--nearest"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Error: --area excludes --nearest" in r.stdout
    r = subprocess.run([split, "0.5", "35", "--image", str(src), "--images", "10", "--resize", "160x120", "--area"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--resize" in r.stdout and "bands are not supported" in r.stdout
