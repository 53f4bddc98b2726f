"""The affine warp on the GPU (mi_blur_enqueue_warp, mi_blur_ctx_set_warp, warp_affine() / rotate(), the host's --rotate):
exact bytes against the numpy restatement of the header's definition (warp_ref.py), and which of the two kernels took
each launch against the restated eligibility rule."""
import subprocess

import numpy as np
import pytest

from resample_harness import (WARP, apps, blocks, check_gpu_context, check_gpu_context_enlarging, check_pointer_offsets, check_synthetic_stream,  # noqa: F401
                              gpu_run, last, read_ppm, spans_tiles, torch_cuda, write_ppm)
from resize_ref import ref_resize
from warp_ref import (BILINEAR, CLAMP, CONSTANT, LIMIT_FILL, LIMIT_MAPS, NEAREST, Q, TILED_SHAPES, edge_image, identity, in_the_admitted_region,
                      limit_out, limit_references, quantise, ref_warp, rotation_m, scale_matrix, takes_tiled)

pytestmark = pytest.mark.gpu

TILED, GENERIC = WARP.tiled, WARP.generic
BORDERS = (CLAMP, CONSTANT)


def maps(w, h):
    """name -> m for a W x H input, all inside the admitted region |m0|+|m1| <= 3Q/2, |m3|+|m4| <= 3Q/2."""
    out = {f"rot{a}": rotation_m(w, h, a) for a in (0, 90, 180, 270, 30, 45, -17.3)}
    out["rot30x0.67"] = rotation_m(w, h, 30.0, 1 / 0.67)            # the forward scale 1.49: the map steps 0.67 pixels
    out["rot-50x1.04"] = rotation_m(w, h, -50.0, 1 / 1.04)
    out["scale1.5"] = quantise([1.5, 0, -7.25, 0, 1.5, 3.5])
    out["scale0.67"] = quantise([0.67, 0, 0.3, 0, 0.67, -0.6])
    out["shear0.5"] = quantise([1.0, 0.5, -20.75, -0.5, 1.0, 30.5])
    out["subpixel"] = [Q, 0, 3 * Q // 8 + 1, 0, Q, -5 * Q // 8 - 1]
    out["negative"] = [Q, 0, -37 * Q + 77, 0, Q, -21 * Q - 5]
    out["far-right"] = identity(w + 70, 0)                           # wholly outside the source: fill, or the clamped edge
    out["far-up-left"] = quantise([0.9, 0.1, -3.0 * w, -0.1, 0.9, -2.5 * h])
    out["half-out"] = rotation_m(w, h, 20.0, 1.0, (0.0, 0.0))
    return out


@pytest.mark.parametrize("case", TILED_SHAPES, ids=lambda c: "x".join(map(str, c[0])) + f"-{c[1][0]}x{c[1][1]}")
def test_aligned_launches_take_the_tiled_kernel(pkg, L, torch_cuda, case):
    shape, (wo, ho) = case
    n, h, w, c = shape
    assert spans_tiles(wo, ho, c)                                   # more than one tile both ways
    img = edge_image(np.random.default_rng(sum(shape)), n, h, w, c)
    for name, m in maps(w, h).items():
        assert in_the_admitted_region(m), name
        for border in BORDERS:
            assert takes_tiled(shape, m, wo, ho, BILINEAR, border), (name, border)
            got = gpu_run(WARP, pkg, L, torch_cuda, img, (m, wo, ho, BILINEAR, border, 173))
            assert last(L) == TILED, (name, border)
            assert np.array_equal(got, ref_warp(img, m, wo, ho, BILINEAR, border, 173)), (name, border)
    # one image at the input's own size
    for name in ("rot0", "rot30", "rot90", "far-right", "half-out"):
        m = maps(w, h)[name]
        one = img[:1]
        got = gpu_run(WARP, pkg, L, torch_cuda, one, (m, w, h, BILINEAR, CONSTANT, 9))
        assert last(L) == TILED and np.array_equal(got, ref_warp(one, m, w, h, BILINEAR, CONSTANT, 9)), name
        if name == "rot0":
            assert np.array_equal(got, one)


def test_xcd_remap_on_and_off(pkg, L, torch_cuda):
    """One batch with 16 or more workgroups and one with fewer, every channel count."""
    rng = np.random.default_rng(11)
    for c in (1, 2, 3, 4):
        for n, (h, w), (wo, ho) in ((1, (40, 64), (64, 40)), (3, (80, 96), (144, 70))):
            assert (blocks(n, wo, ho, c) >= 16) == (n == 3)
            img = edge_image(rng, n, h, w, c)
            m = rotation_m(w, h, 33.0, 1.1)
            got = gpu_run(WARP, pkg, L, torch_cuda, img, (m, wo, ho, BILINEAR, CONSTANT, 60))
            assert last(L) == TILED and np.array_equal(got, ref_warp(img, m, wo, ho, BILINEAR, CONSTANT, 60)), (c, n)


def test_exact_right_angles_and_the_identity(pkg, L, torch_cuda):
    img = np.random.default_rng(12).integers(0, 256, size=(2, 64, 96, 4), dtype=np.uint8)
    for border in BORDERS:
        assert np.array_equal(gpu_run(WARP, pkg, L, torch_cuda, img, (identity(), 96, 64, BILINEAR, border, 0)), img) and last(L) == TILED
        got = gpu_run(WARP, pkg, L, torch_cuda, img, ([0, -Q, 95 * Q, Q, 0, 0], 64, 96, BILINEAR, border, 0))
        assert last(L) == TILED and np.array_equal(got, np.rot90(img, 1, axes=(1, 2)))


def test_other_launches_take_the_generic_kernel(pkg, L, torch_cuda):
    rng = np.random.default_rng(3)
    # NEAREST on an aligned shape; 5 channels; input rows, then output rows, that are no multiple of 16 bytes; tiny shapes
    cases = [((2, 80, 96, 4), (132, 70), NEAREST), ((1, 24, 64, 5), (128, 48), BILINEAR), ((1, 17, 33, 3), (48, 29), BILINEAR),
             ((1, 17, 32, 3), (50, 29), BILINEAR), ((1, 1, 1, 3), (9, 9), BILINEAR), ((2, 9, 5, 1), (11, 17), BILINEAR), ((1, 40, 50, 2), (1, 1), NEAREST)]
    for shape, (wo, ho), mode in cases:
        n, h, w, c = shape
        img = edge_image(rng, n, h, w, c)
        for m in (rotation_m(w, h, 30.0), rotation_m(w, h, -100.0, 0.8, (1.0, 2.0)), identity(w + 3, -2), quantise([1.0, 0.5, -0.75 * w, 0.25, 1.0, 0.4 * h])):
            for border in BORDERS:
                assert not takes_tiled(shape, m, wo, ho, mode, border)
                got = gpu_run(WARP, pkg, L, torch_cuda, img, (m, wo, ho, mode, border, 99))
                assert last(L) == GENERIC, (shape, wo, ho, mode)
                assert np.array_equal(got, ref_warp(img, m, wo, ho, mode, border, 99)), (shape, m, wo, ho, mode, border)
    # aligned shape, pointers off 16 bytes: guards checked inside gpu_run
    img = edge_image(rng, 2, 35, 48, 2)
    check_pointer_offsets(WARP, pkg, L, torch_cuda, img, (rotation_m(48, 35, 30.0), 56, 70, BILINEAR, CONSTANT, 5))


def test_a_footprint_over_64_kib_takes_the_generic_kernel(pkg, L, torch_cuda):
    """An 8x reduction of a one-channel image: a 64 x 32 pixel tile reads 512 x 256 input pixels, 128 KiB."""
    shape = (1, 512, 512, 1)
    img = np.random.default_rng(8).integers(0, 256, size=shape, dtype=np.uint8)
    m = scale_matrix(1, 8)
    for border in BORDERS:
        assert not takes_tiled(shape, m, 64, 64, BILINEAR, border)
        got = gpu_run(WARP, pkg, L, torch_cuda, img, (m, 64, 64, BILINEAR, border, 0))
        assert last(L) == GENERIC and np.array_equal(got, ref_warp(img, m, 64, 64, BILINEAR, border))
    assert np.array_equal(ref_warp(img, m, 64, 64, BILINEAR, CLAMP), ref_resize(img, 64, 64))
    # a 4x reduction still fits (256 x 128 pixels of one byte: 32 KiB), outside the admitted region: the walk decides
    m4 = scale_matrix(1, 4)
    assert not in_the_admitted_region(m4) and takes_tiled(shape, m4, 128, 128, BILINEAR, CLAMP)
    got = gpu_run(WARP, pkg, L, torch_cuda, img, (m4, 128, 128, BILINEAR, CLAMP, 0))
    assert last(L) == TILED and np.array_equal(got, ref_resize(img, 128, 128))


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_maps_at_the_limits_of_the_header(pkg, L, torch_cuda, c):
    """Linear coefficients of 2^26 and translations of 2^46 in every sign, zero and rank-one linear parts, steps of 1 / 65536
    pixel (LIMIT_MAPS), on two 64 x 64 images with distinct corners and edges: at most 16 KiB, so the whole image fits the
    LDS and every BILINEAR launch is tiled.  limit_references() asserts, on the reference alone, that these outputs tell a
    right kernel from one that writes `fill` or a wrong corner."""
    img, refs = limit_references(2, c)
    wo, ho = limit_out(c)
    for name, (m, _, _) in LIMIT_MAPS.items():
        for border in BORDERS:
            assert takes_tiled(img.shape, m, wo, ho, BILINEAR, border), (name, border)
            for mode, kernel in ((BILINEAR, TILED), (NEAREST, GENERIC)):
                got = gpu_run(WARP, pkg, L, torch_cuda, img, (m, wo, ho, mode, border, LIMIT_FILL))
                assert last(L) == kernel, (name, border, mode)
                assert np.array_equal(got, refs[name, mode, border]), (name, border, mode)


def test_x2_clamp_warp_equals_the_resize(pkg, L, torch_cuda):
    img = np.random.default_rng(9).integers(0, 256, size=(2, 45, 64, 3), dtype=np.uint8)
    got = gpu_run(WARP, pkg, L, torch_cuda, img, (scale_matrix(2, 1), 128, 90, BILINEAR, CLAMP, 0))
    assert last(L) == TILED
    assert np.array_equal(got, pkg.resize(img, (128, 90)))
    assert L.mi_blur_last_kernel().decode() == "blur_resize_tiled_kernel"


def test_gpu_equals_cpu_device_on_the_synthetic_stream(pkg, L, torch_cuda):
    cases = ((rotation_m(320, 240, 30.0), (320, 240), CONSTANT), (quantise([0.8, 0.3, -20.5, -0.2, 0.7, 31.25]), (400, 300), CLAMP),
             (scale_matrix(1, 2), (160, 120), CLAMP))
    check_synthetic_stream(WARP, pkg, L, torch_cuda, [(m, wo, ho, mode, border, 128) for m, (wo, ho), border in cases for mode in (BILINEAR, NEAREST)])


@pytest.mark.parametrize("target", [(160, 120), (100, 75)], ids=lambda t: "x".join(map(str, t)))
def test_gpu_context(pkg, L, torch_cuda, target):
    shape = (6, 120, 160, 3)
    n, h, w, c = shape
    wo, ho = target
    img = np.random.default_rng(13).integers(0, 256, size=shape, dtype=np.uint8)
    m = rotation_m(w, h, 30.0)
    kernel = TILED if takes_tiled(shape, m, wo, ho) else GENERIC
    assert (kernel == TILED) == (target == (160, 120))              # 100 x 3 bytes is no whole number of chunks
    check_gpu_context(WARP, pkg, L, img, (m, wo, ho, BILINEAR, CONSTANT, 40), kernel)


def test_gpu_context_enlarging(pkg, L, torch_cuda):
    """160 x 120 to 320 x 240, rotated: the output is four times the input, so slots sized by the input would be overrun."""
    shape = (6, 120, 160, 3)
    n, h, w, c = shape
    wo, ho = 320, 240
    img = np.random.default_rng(14).integers(0, 256, size=shape, dtype=np.uint8)
    m = rotation_m(w, h, 30.0, 2.0)
    check_gpu_context_enlarging(WARP, pkg, L, img, (m, wo, ho, BILINEAR, CONSTANT, 40), fill=40)


def test_numpy_functions_on_the_gpu(pkg, L, torch_cuda):
    rng = np.random.default_rng(17)
    stack = rng.integers(0, 256, size=(3, 90, 128, 3), dtype=np.uint8)
    assert np.array_equal(pkg.rotate(stack, 30.0), ref_warp(stack, rotation_m(128, 90, 30.0), 128, 90))
    assert np.array_equal(pkg.rotate(stack, -45.0, 1.2, dsize=(200, 61), border="clamp", batch=2), ref_warp(stack, rotation_m(128, 90, -45.0, 1.2), 200, 61, BILINEAR, CLAMP))
    assert np.array_equal(pkg.rotate(stack[0], 10.0, mode="nearest", fill=200, batch=1), ref_warp(stack[:1], rotation_m(128, 90, 10.0), 128, 90, NEAREST, CONSTANT, 200)[0])
    M = [[0.9, 0.2, 5.5], [-0.1, 1.1, -3.25]]
    assert np.array_equal(pkg.warp_affine(stack, M, (160, 100), inverse=True, fill=17), ref_warp(stack, quantise(M[0] + M[1]), 160, 100, BILINEAR, CONSTANT, 17))
    odd = rng.integers(0, 256, size=(45, 71), dtype=np.uint8)
    assert np.array_equal(pkg.rotate(odd, 75.0), ref_warp(odd[None, :, :, None], rotation_m(71, 45, 75.0), 71, 45)[0, :, :, 0])


def test_host_rotate(pkg, apps, torch_cuda, tmp_path):
    het, split = apps
    img = np.random.default_rng(19).integers(0, 256, size=(240, 320, 3), dtype=np.uint8)
    src = tmp_path / "in.ppm"
    write_ppm(src, img)
    m = rotation_m(320, 240, 30.0)
    for flags, mode, border, fill, name in (([], BILINEAR, CLAMP, 0, "bilinear"), (["--border-fill", "90"], BILINEAR, CONSTANT, 90, "bilinear"),
                                            (["--nearest"], NEAREST, CLAMP, 0, "nearest")):
        want = ref_warp(img[None], m, 320, 240, mode, border, fill)[0]
        for run in (["gpu", "1.0", "35"], ["both", "0.7", "35"]):
            dst = tmp_path / f"{run[0]}_{name}_{fill}.ppm"
            r = subprocess.run([het, *run, "--image", str(src), "--images", "100", "--rotate", "30", *flags, "--save", str(dst)],
                               capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            assert f"Blur kernel: {name} warp, rotate 30 deg, 320x240 -> 320x240" in r.stdout
            got = read_ppm(dst)
            assert got.shape == (240, 320, 3) and np.array_equal(got, want), (run, name, fill)
    r = subprocess.run([split, "0.5", "35", "--image", str(src), "--images", "10", "--rotate", "30"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--rotate" in r.stdout and "bands are not supported" in r.stdout
