"""The perspective warp on the GPU (mi_blur_enqueue_warp_perspective, mi_blur_ctx_set_warp_perspective,
warp_perspective(), the host's --perspective): exact bytes against the numpy restatement of the header's definition
(warp_perspective_ref.py), and which of the two kernels took each launch against the restated eligibility rule."""
import subprocess

import numpy as np
import pytest

from resample_harness import (PERSP, apps, blocks, check_gpu_context, check_gpu_context_enlarging, check_pointer_offsets, check_synthetic_stream,  # noqa: F401
                              gpu_run, last, read_ppm, torch_cuda, write_ppm)
from warp_ref import LIMIT_FILL, NARROW_HEIGHTS, NARROW_N, NARROW_ROWS, TILED_SHAPES, edge_image, impulse_rows, limit_out
from warp_perspective_ref import (BIG_QUAD, BILINEAR, CLAMP, CONSTANT, EXTREME, LIMIT_MAPS, NEAREST, Q, affine_h, limit_references, max_footprint,
                                  named_maps, named_quads, out_corners, quad_h, ref_warp, set_matrix, takes_tiled, valid)

pytestmark = pytest.mark.gpu

TILED, GENERIC = PERSP.tiled, PERSP.generic
BORDERS = (CLAMP, CONSTANT)


@pytest.mark.parametrize("case", TILED_SHAPES, ids=lambda c: "x".join(map(str, c[0])) + f"-{c[1][0]}x{c[1][1]}")
def test_aligned_launches_take_the_tiled_kernel(pkg, L, torch_cuda, case):
    shape, (wo, ho) = case
    n, h, w, c = shape
    img = edge_image(np.random.default_rng(sum(shape)), n, h, w, c)
    for name, hh in named_maps(w, h, wo, ho).items():
        for border in BORDERS:
            assert valid(hh, wo, ho) and takes_tiled(shape, hh, wo, ho, BILINEAR, border), (name, border)
            got = gpu_run(PERSP, pkg, L, torch_cuda, img, (hh, wo, ho, BILINEAR, border, 173))
            assert last(L) == TILED, (name, border)
            assert np.array_equal(got, ref_warp(img, hh, wo, ho, BILINEAR, border, 173)), (name, border)


def test_xcd_remap_on_and_off(pkg, L, torch_cuda):
    """One batch with 16 or more workgroups and one with fewer, every channel count."""
    rng = np.random.default_rng(11)
    for c in (1, 2, 3, 4):
        for n, (h, w), (wo, ho) in ((1, (40, 64), (64, 40)), (3, (80, 96), (144, 70))):
            assert (blocks(n, wo, ho, c) >= 16) == (n == 3)
            img = edge_image(rng, n, h, w, c)
            hh = named_maps(w, h, wo, ho)["tilt"]
            assert takes_tiled(img.shape, hh, wo, ho)
            got = gpu_run(PERSP, pkg, L, torch_cuda, img, (hh, wo, ho, BILINEAR, CONSTANT, 60))
            assert last(L) == TILED and np.array_equal(got, ref_warp(img, hh, wo, ho, BILINEAR, CONSTANT, 60)), (c, n)


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_maps_at_the_limits_of_the_header(pkg, L, torch_cuda, c):
    """LIMIT_MAPS of warp_perspective_ref.py (D = 1, entries of 2^32 and 2^48, quotients near 2^60, steps of 2^-42) on two
    64 x 64 images: the whole image fits the LDS, so every BILINEAR launch is tiled and every NEAREST one generic."""
    img, refs = limit_references(2, c)
    wo, ho = limit_out(c)
    for name, (hf, _, _, _) in LIMIT_MAPS.items():
        hh = hf(wo)
        for border in BORDERS:
            assert takes_tiled(img.shape, hh, wo, ho, BILINEAR, border), (name, border)
            for mode, kernel in ((BILINEAR, TILED), (NEAREST, GENERIC)):
                got = gpu_run(PERSP, pkg, L, torch_cuda, img, (hh, wo, ho, mode, border, LIMIT_FILL))
                assert last(L) == kernel, (name, border, mode)
                assert np.array_equal(got, refs[name, mode, border]), (name, border, mode)


def test_other_launches_take_the_generic_kernel(pkg, L, torch_cuda):
    rng = np.random.default_rng(3)
    # NEAREST on an aligned shape; 5 channels; input rows, then output rows, that are no multiple of 16 bytes; 1 x 1 in and out
    cases = [((2, 80, 96, 4), (132, 70), NEAREST), ((1, 24, 64, 5), (128, 48), BILINEAR), ((1, 17, 33, 3), (48, 29), BILINEAR),
             ((1, 17, 32, 3), (50, 29), BILINEAR), ((1, 1, 1, 3), (9, 9), BILINEAR), ((1, 40, 50, 2), (1, 1), NEAREST)]
    for shape, (wo, ho), mode in cases:
        n, h, w, c = shape
        img = edge_image(rng, n, h, w, c)
        maps = [affine_h([Q, 0, -3 * Q // 8, 0, Q, 5 * Q // 8]), [3, 0, -7, 0, 2, 5, 0, 0, 1], [Q, 0, 0, 0, Q, 0, Q // 64, Q // 128, Q]]
        if wo > 1 and w > 1:
            maps.append(named_maps(w, h, wo, ho)["keystone"])
        for hh in maps:
            for border in BORDERS:
                assert valid(hh, wo, ho) and not takes_tiled(shape, hh, wo, ho, mode, border)
                got = gpu_run(PERSP, pkg, L, torch_cuda, img, (hh, wo, ho, mode, border, 99))
                assert last(L) == GENERIC, (shape, wo, ho, mode)
                assert np.array_equal(got, ref_warp(img, hh, wo, ho, mode, border, 99)), (shape, hh, wo, ho, mode, border)
    # aligned shape, pointers off 16 bytes: guards checked inside gpu_run
    img = edge_image(rng, 2, 35, 48, 2)
    check_pointer_offsets(PERSP, pkg, L, torch_cuda, img, (named_maps(48, 35, 56, 70)["tilt"], 56, 70, BILINEAR, CONSTANT, 5))


def test_a_footprint_over_64_kib_takes_the_generic_kernel(pkg, L, torch_cuda):
    """A trapezoid of a 512 x 512 one-channel image to 64 x 64: a tile of the wide end stages 161 280 bytes, so the whole
    launch is generic; to 128 x 128 the largest tile stages 45 824 bytes and the launch is tiled."""
    shape = (1, 512, 512, 1)
    img = np.random.default_rng(8).integers(0, 256, size=shape, dtype=np.uint8)
    for size, kernel, stages in ((64, GENERIC, 161280), (128, TILED, 45824)):
        hh = quad_h(512, 512, size, size, BIG_QUAD)
        for border in BORDERS:
            assert max_footprint(shape, hh, size, size, border) == stages and takes_tiled(shape, hh, size, size, BILINEAR, border) == (kernel == TILED)
            got = gpu_run(PERSP, pkg, L, torch_cuda, img, (hh, size, size, BILINEAR, border, 0))
            assert last(L) == kernel and np.array_equal(got, ref_warp(img, hh, size, size, BILINEAR, border)), (size, border)


@pytest.mark.parametrize("case", EXTREME, ids=lambda c: "x".join(map(str, c[0])))
def test_extreme_shapes(pkg, L, torch_cuda, case):
    ishape, (wo, ho), hh, border = case
    img = np.random.default_rng(5).integers(0, 256, size=(1,) + ishape, dtype=np.uint8)
    for b in BORDERS if border is None else (border,):
        assert valid(hh, wo, ho) and takes_tiled(img.shape, hh, wo, ho, BILINEAR, b)
        got = gpu_run(PERSP, pkg, L, torch_cuda, img, (hh, wo, ho, BILINEAR, b, 7))
        assert last(L) == TILED and np.array_equal(got, ref_warp(img, hh, wo, ho, BILINEAR, b, 7)), b


def test_one_chunk_inputs(pkg, L, torch_cuda):
    """warp_ref's NARROW_ROWS inputs (one 16-byte chunk per row; one group of three for 3 channels) with `keystone`: the
    staged box is the whole row, or the whole image."""
    rng = np.random.default_rng(78)
    for w, c in NARROW_ROWS:
        wo, ho = (132 if c == 4 else 144), 33
        for h in NARROW_HEIGHTS:
            img = impulse_rows(rng, NARROW_N, h, w, c)
            hh = named_maps(w, max(h, 2), wo, ho)["keystone"]
            for border in BORDERS:
                assert valid(hh, wo, ho) and takes_tiled(img.shape, hh, wo, ho, BILINEAR, border), (w, c, h)
                got = gpu_run(PERSP, pkg, L, torch_cuda, img, (hh, wo, ho, BILINEAR, border, 173))
                assert last(L) == TILED and np.array_equal(got, ref_warp(img, hh, wo, ho, BILINEAR, border, 173)), (w, c, h, border)


def test_gpu_equals_cpu_device_on_the_synthetic_stream(pkg, L, torch_cuda):
    cases = (("keystone", (320, 240), CONSTANT), ("tilt", (400, 300), CLAMP), ("half-out", (160, 120), CLAMP))
    check_synthetic_stream(PERSP, pkg, L, torch_cuda, [(named_maps(320, 240, wo, ho)[name], wo, ho, mode, border, 128)
                                                       for name, (wo, ho), border in cases for mode in (BILINEAR, NEAREST)])


@pytest.mark.parametrize("target", [(160, 120), (100, 75)], ids=lambda t: "x".join(map(str, t)))
def test_gpu_context(pkg, L, torch_cuda, target):
    shape = (6, 120, 160, 3)
    n, h, w, c = shape
    wo, ho = target
    img = np.random.default_rng(13).integers(0, 256, size=shape, dtype=np.uint8)
    hh = named_maps(w, h, wo, ho)["tilt"]
    kernel = TILED if takes_tiled(shape, hh, wo, ho) else GENERIC
    assert (kernel == TILED) == (target == (160, 120))              # 100 x 3 bytes is no whole number of chunks
    check_gpu_context(PERSP, pkg, L, img, (hh, wo, ho, BILINEAR, CONSTANT, 40), kernel)


def test_gpu_context_enlarging(pkg, L, torch_cuda):
    """160 x 120 to 320 x 240 through a quad: the output is four times the input, so slots sized by the input would be overrun."""
    shape = (6, 120, 160, 3)
    n, h, w, c = shape
    wo, ho = 320, 240
    img = np.random.default_rng(14).integers(0, 256, size=shape, dtype=np.uint8)
    hh = named_maps(w, h, wo, ho)["keystone"]
    check_gpu_context_enlarging(PERSP, pkg, L, img, (hh, wo, ho, BILINEAR, CONSTANT, 40), fill=40)


def test_numpy_functions_on_the_gpu(pkg, L, torch_cuda):
    rng = np.random.default_rng(17)
    stack = rng.integers(0, 256, size=(3, 90, 128, 3), dtype=np.uint8)
    quad = named_quads(128, 90)["tilt"]
    for dsize, mode, mo, border, bo, fill, batch in ((None, "bilinear", BILINEAR, "constant", CONSTANT, 0, 0), ((200, 61), "bilinear", BILINEAR, "clamp", CLAMP, 0, 2),
                                                     ((128, 90), "nearest", NEAREST, "constant", CONSTANT, 200, 1)):
        wo, ho = dsize or (128, 90)
        M = pkg.perspective_matrix(quad, out_corners(wo, ho))
        hh = set_matrix([v for row in M for v in row], False, wo, ho)[0]
        got = pkg.warp_perspective(stack, M, dsize, mode, border, fill, batch=batch)
        assert np.array_equal(got, ref_warp(stack, hh, wo, ho, mo, bo, fill)), (dsize, mode, border)
    inv = [1.0, 0.1, -3.0, 0.05, 0.9, 2.0, 1e-4, -2e-4, 1.0]
    odd = rng.integers(0, 256, size=(45, 71), dtype=np.uint8)
    assert np.array_equal(pkg.warp_perspective(odd, np.array(inv).reshape(3, 3), inverse=True, fill=17),
                          ref_warp(odd[None, :, :, None], set_matrix(inv, True, 71, 45)[0], 71, 45, BILINEAR, CONSTANT, 17)[0, :, :, 0])


def test_host_perspective(pkg, apps, torch_cuda, tmp_path):
    het, split = apps
    img = np.random.default_rng(19).integers(0, 256, size=(240, 320, 3), dtype=np.uint8)
    src = tmp_path / "in.ppm"
    write_ppm(src, img)
    quad = named_quads(320, 240)["keystone"]
    arg = ",".join(repr(float(v)) for p in quad for v in p)
    hh = quad_h(320, 240, 320, 240, quad)
    for flags, mode, border, fill, name in (([], BILINEAR, CLAMP, 0, "bilinear"), (["--border-fill", "90"], BILINEAR, CONSTANT, 90, "bilinear"),
                                            (["--nearest"], NEAREST, CLAMP, 0, "nearest")):
        want = ref_warp(img[None], hh, 320, 240, mode, border, fill)[0]
        for run in (["gpu", "1.0", "35"], ["both", "0.7", "35"]):
            dst = tmp_path / f"{run[0]}_{name}_{fill}.ppm"
            r = subprocess.run([het, *run, "--image", str(src), "--images", "100", "--perspective", arg, *flags, "--save", str(dst)],
                               capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            assert f"Blur kernel: {name} warp, perspective, 320x240 -> 320x240" in r.stdout
            got = read_ppm(dst)
            assert got.shape == (240, 320, 3) and np.array_equal(got, want), (run, name, fill)
    r = subprocess.run([split, "0.5", "35", "--image", str(src), "--images", "10", "--perspective", arg], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--perspective" in r.stdout and "bands are not supported" in r.stdout
