"""The image resize on the GPU (mi_blur_enqueue_resize, mi_blur_ctx_set_resize, resize(), the hosts' --resize): exact bytes
against the numpy restatement of the header's definition (resize_ref.py), and which of the two kernels took each launch."""
import subprocess

import numpy as np
import pytest

from resample_harness import (RESIZE, apps, check_gpu_context, check_pointer_offsets, check_synthetic_stream, gpu_run, last, pinned, read_ppm,  # noqa: F401
                              spans_tiles, torch_cuda, write_ppm)
from resize_ref import BILINEAR, NEAREST, ref_axis, ref_resize, takes_tiled, tile_geometry

pytestmark = pytest.mark.gpu

TILED, GENERIC = RESIZE.tiled, RESIZE.generic
MODES = (BILINEAR, NEAREST)


@pytest.mark.parametrize("case", [((2, 33, 32, 1), 64, 66, False), ((1, 33, 48, 3), 96, 67, False), ((2, 35, 48, 2), 56, 35, False),
                                  ((1, 20, 64, 4), 64, 53, False), ((1, 40, 176, 3), 704, 70, True), ((1, 17, 16, 1), 1088, 97, True),
                                  ((1, 70, 704, 3), 704, 70, True)],
                         ids=lambda c: "x".join(map(str, c[0])) + f"-{c[1]}x{c[2]}")
def test_aligned_enlargements_take_the_tiled_kernel(pkg, L, torch_cuda, case):
    """Both axes, x only, y only, a large ratio, the same size; the last three span more than one tile both ways."""
    shape, wo, ho, many_tiles = case
    assert takes_tiled(shape, wo, ho) and spans_tiles(wo, ho, shape[3], tile_geometry) == many_tiles
    img = np.random.default_rng(sum(shape) + wo).integers(0, 256, size=shape, dtype=np.uint8)
    got = gpu_run(RESIZE, pkg, L, torch_cuda, img, (wo, ho, BILINEAR))
    assert last(L) == TILED, case
    assert np.array_equal(got, ref_resize(img, wo, ho)), case
    if (wo, ho) == (shape[2], shape[1]):
        assert np.array_equal(got, img)                              # same size: the identity, through the tiled kernel


def seam_images(rng, h, w, c, wo, ho):
    """In the manner of test_sep_down_gpu.seam_images, for OUTPUT tiles: low-amplitude noise with 0 / 255 impulses (one
    channel each) and 0 / 255 step edges at the input pixels under every seam between output tiles (the a and b of
    the output rows and columns either side of it) and on the borders; an all-255 image; impulses in the four corners."""
    ncols, cpr, trows = tile_geometry(wo, ho, c)
    xa, xb, _ = ref_axis(w, wo)
    ya, yb, _ = ref_axis(h, ho)
    orows = [y for s in range(trows, ho, trows) for y in (s - 1, s)]
    ocols = [x for s in range(ncols, cpr, ncols) for x in ((s * 16 - 1) // c, min(-(-s * 16 // c), wo - 1))]
    rows = sorted({0, h - 1} | {int(v) for y in orows for v in (ya[y], yb[y])})
    cols = sorted({0, w - 1} | {int(v) for x in ocols for v in (xa[x], xb[x])})
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


@pytest.mark.parametrize("case", [(35, 352, 3, 704, 70), (49, 544, 1, 1088, 98), (33, 80, 4, 160, 66),                # 2x
                                  (31, 352, 1, 800, 70), (31, 176, 3, 400, 70), (31, 176, 1, 400, 70), (40, 96, 2, 264, 45)],   # 176 -> 400 and the like
                         ids=lambda c: "x".join(map(str, c[:3])) + f"-{c[3]}x{c[4]}")
def test_tile_seams(pkg, L, torch_cuda, case):
    h, w, c, wo, ho = case
    ncols, cpr, trows = tile_geometry(wo, ho, c)
    assert ho > trows and (cpr > ncols or (w, c, wo) == (176, 1, 400))   # more than one tile both ways (176 -> 400 x 1 channel: 25 chunks, rows only)
    img = seam_images(np.random.default_rng(7), h, w, c, wo, ho)
    assert takes_tiled(img.shape, wo, ho)
    got = gpu_run(RESIZE, pkg, L, torch_cuda, img, (wo, ho, BILINEAR))
    assert last(L) == TILED
    assert (got[2] == 255).all(), case
    assert np.array_equal(got, ref_resize(img, wo, ho)), case


def test_other_launches_take_the_generic_kernel(pkg, L, torch_cuda):
    rng = np.random.default_rng(3)
    cases = [((1, 24, 64, 5), 128, 48), ((1, 50, 7, 5), 21, 75), ((1, 17, 33, 3), 50, 29), ((1, 17, 32, 3), 50, 29), ((1, 17, 33, 3), 64, 29),
             ((1, 1, 1, 3), 9, 9), ((1, 100, 100, 1), 1, 1), ((2, 9, 5, 1), 11, 17)]
    for shape, wo, ho in cases:
        img = rng.integers(0, 256, size=shape, dtype=np.uint8)
        for mode in MODES:
            assert not takes_tiled(shape, wo, ho, mode)
            got = gpu_run(RESIZE, pkg, L, torch_cuda, img, (wo, ho, mode))
            assert last(L) == GENERIC, (shape, wo, ho, mode)
            assert np.array_equal(got, ref_resize(img, wo, ho, mode)), (shape, wo, ho, mode)
    img = rng.integers(0, 256, size=(2, 35, 48, 2), dtype=np.uint8)              # aligned shape, pointers off 16 bytes
    check_pointer_offsets(RESIZE, pkg, L, torch_cuda, img, (112, 70, BILINEAR))


def test_reductions_and_nearest(pkg, L, torch_cuda):
    """Bytes, and the kernel takes_tiled() predicts: reductions on either or both axes, NEAREST at every ratio."""
    rng = np.random.default_rng(4)
    for shape in ((2, 64, 96, 2), (1, 48, 64, 3), (1, 33, 40, 3)):
        n, h, w, c = shape
        img = rng.integers(0, 256, size=shape, dtype=np.uint8)
        for wo, ho in ((w, h), (2 * w, 2 * h), (w // 2, h // 2), (w * 2 // 3 // 16 * 16 + 16, h), (w, h - 1), (2 * w, h // 2), (w // 4, 3 * h), (3 * w, 3 * h), (1, 1)):
            for mode in MODES:
                got = gpu_run(RESIZE, pkg, L, torch_cuda, img, (wo, ho, mode))
                assert last(L) == (TILED if takes_tiled(shape, wo, ho, mode) else GENERIC), (shape, wo, ho, mode)
                assert np.array_equal(got, ref_resize(img, wo, ho, mode)), (shape, wo, ho, mode)
    img = rng.integers(0, 256, size=(1, 20, 32, 1), dtype=np.uint8)
    for k in (2, 3):
        assert np.array_equal(gpu_run(RESIZE, pkg, L, torch_cuda, img, (32 * k, 20 * k, NEAREST)), np.repeat(np.repeat(img, k, axis=1), k, axis=2))


def test_gpu_equals_cpu_device_on_the_synthetic_stream(pkg, L, torch_cuda):
    check_synthetic_stream(RESIZE, pkg, L, torch_cuda, [(wo, ho, mode) for wo, ho in ((640, 480), (427, 320), (200, 150)) for mode in MODES])


@pytest.mark.parametrize("target", [(320, 240), (100, 75)], ids=lambda t: "x".join(map(str, t)))
def test_gpu_context(pkg, L, torch_cuda, target):
    shape = (6, 120, 160, 3)
    n, h, w, c = shape
    wo, ho = target
    img = np.random.default_rng(13).integers(0, 256, size=shape, dtype=np.uint8)
    kernel = TILED if takes_tiled(shape, wo, ho) else GENERIC
    assert (kernel == TILED) == (target == (320, 240))
    check_gpu_context(RESIZE, pkg, L, img, (wo, ho, BILINEAR), kernel)
    # a context without the setter is what it was: the same pinned submit gives the box blur, and a pinned submit
    # above the batch server's threshold (zero_copy_server_min_kb, 1280 KiB of output: these 6 frames are 338 KiB,
    # which has always been one launch, so four times the batch) still takes blur_server_kernel
    box = np.empty_like(img)
    assert L.mi_blur_cpu_run(img.ctypes.data, box.ctypes.data, w, h, c, 1, n, 4) == pkg.OK
    with pinned(L, img.size, img.size, 4 * img.size, 4 * img.size) as ((pin_in, a), (pin_out, b), (big_in, ba), (big_out, bb)):
        with pkg.Context(0, w, h, c, 1, max_batch=4 * n, n_slots=3) as plain:
            a[:] = img.reshape(-1)
            b[:] = 0
            plain.submit(pin_in, pin_out, n)
            plain.sync()
            assert np.array_equal(b.reshape(img.shape), box)
            ba, bb = ba.reshape((4,) + img.shape), bb.reshape((4,) + img.shape)
            ba[:] = img
            bb[:] = 0
            assert 4 * img.size >= 1280 * 1024
            plain.submit(big_in, big_out, 4 * n)
            plain.sync()
            assert last(L) == "blur_server_kernel"
            assert all(np.array_equal(bb[i], box) for i in range(4))


def test_numpy_function_on_the_gpu(pkg, L, torch_cuda):
    rng = np.random.default_rng(17)
    stack = rng.integers(0, 256, size=(3, 90, 128, 3), dtype=np.uint8)
    assert np.array_equal(pkg.resize(stack, (256, 180)), ref_resize(stack, 256, 180))
    assert np.array_equal(pkg.resize(stack, (200, 61), batch=2), ref_resize(stack, 200, 61))
    assert np.array_equal(pkg.resize(stack[0], (256, 180), "nearest", batch=1), ref_resize(stack[:1], 256, 180, NEAREST)[0])
    assert np.array_equal(pkg.resize(stack[0], (90, 40)), ref_resize(stack[:1], 90, 40)[0])
    odd = rng.integers(0, 256, size=(45, 71), dtype=np.uint8)
    assert np.array_equal(pkg.resize(odd, (150, 100)), ref_resize(odd[None, :, :, None], 150, 100)[0, :, :, 0])
    even = rng.integers(0, 256, size=(45, 64), dtype=np.uint8)
    assert np.array_equal(pkg.resize(even, (128, 90)), ref_resize(even[None, :, :, None], 128, 90)[0, :, :, 0])


def test_hosts_resize(pkg, apps, torch_cuda, tmp_path):
    het, split = apps
    rng = np.random.default_rng(19)
    img = rng.integers(0, 256, size=(240, 320, 3), dtype=np.uint8)
    src = tmp_path / "in.ppm"
    write_ppm(src, img)
    for flags, mode, name in (([], BILINEAR, "bilinear"), (["--nearest"], NEAREST, "nearest")):
        want = ref_resize(img[None], 640, 480, mode)[0]
        for run in (["gpu", "1.0", "35"], ["both", "0.7", "35"]):
            dst = tmp_path / f"{run[0]}_{name}.ppm"
            r = subprocess.run([het, *run, "--image", str(src), "--images", "100", "--resize", "640x480", *flags, "--save", str(dst)],
                               capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            assert f"Blur kernel: {name} resize, 320x240 -> 640x480" in r.stdout
            got = read_ppm(dst)
            assert got.shape == (480, 640, 3) and np.array_equal(got, want), (run, name)
    r = subprocess.run([split, "0.5", "35", "--image", str(src), "--images", "10", "--resize", "640x480"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--resize" in r.stdout and "bands are not supported" in r.stdout
    for extra in (["--sigma", "1.0"], ["--median", "3"], ["--erode", "3"], ["--dilate", "3"], ["--morph-gradient", "3"], ["--bilateral", "5"], ["--conv", "sobel"], ["--pyr-down"], ["--resident"], ["--ksize", "5"],
                  ["--frames", str(tmp_path)]):
        r = subprocess.run([het, "gpu", "1.0", "35", "--image", str(src), "--images", "10", "--resize", "640x480", *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "Error: --resize excludes" in r.stdout, extra
    r = subprocess.run([het, "gpu", "1.0", "35", "--image", str(src), "--images", "10", "--nearest"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Error: --nearest needs --resize" in r.stdout
