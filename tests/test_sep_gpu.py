"""Separable kernels of any radius on a real MI355X (-m gpu): mi_blur_enqueue_sep / _band, a context given a kernel by
mi_blur_ctx_set_kernel, gaussian_blur() and the hosts' --sigma, bit-exact against a numpy restatement of the definition
in include/mi_blur.h (sep_ref.py: edge padding + exact int64 sums), and the binomial taps against the committed golden hashes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from filter_harness import (SEP, apps, check_batch_over_2gib, check_gpu_band_split_equals_whole, check_gpu_context,  # noqa: F401
                            check_unaligned_pointers, gpu_run, read_ppm, torch_cuda, write_ppm)
from sep_ref import rand_taps, ref_sep

pytestmark = pytest.mark.gpu


def gpu_sep(pkg, L, torch, host, wx, wy, **kw):
    return gpu_run(SEP, pkg, L, torch, host, pkg.SepKernel.from_taps(wx, wy), **kw)


# aligned rows (tiled kernel) and everything else (generic kernel)
TILED_SHAPES = [(2, 64, 80, 3), (1, 40, 64, 4), (3, 33, 16, 1), (1, 100, 1024, 1), (1, 37, 2000, 4), (2, 70, 96, 2),
                (1, 1, 16, 1), (1, 2, 48, 1), (1, 300, 512, 3)]
GENERIC_SHAPES = [(1, 17, 33, 3), (2, 30, 250, 3), (1, 9, 5, 1), (1, 31, 29, 2), (1, 50, 7, 5), (1, 24, 64, 5), (1, 1, 1, 3)]
RADII = [(0, 0), (1, 1), (2, 2), (3, 5), (4, 0), (0, 4), (5, 8), (8, 3), (9, 9), (12, 16), (16, 16), (16, 1)]


def test_enqueue_sep_matches_numpy(pkg, L, torch_cuda):
    rng = np.random.default_rng(2024)
    for shapes, kern in ((TILED_SHAPES, SEP.fast), (GENERIC_SHAPES, SEP.generic)):
        for (n, h, w, c) in shapes:
            img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
            for rx, ry in RADII:
                wx, wy = rand_taps(rng, rx, int(rng.integers(0, 9))), rand_taps(rng, ry, int(rng.integers(0, 9)))
                got = gpu_sep(pkg, L, torch_cuda, img, wx, wy)
                assert L.mi_blur_last_kernel().decode() == kern, (n, h, w, c)
                assert np.array_equal(got, ref_sep(img, wx, wy)), ((n, h, w, c), wx, wy)


def test_enqueue_sep_unaligned_pointers(pkg, L, torch_cuda):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(2, 40, 64, 3), dtype=np.uint8)
    k = pkg.SepKernel.from_taps(rand_taps(rng, 6, 8), rand_taps(rng, 3, 8))
    check_unaligned_pointers(SEP, pkg, L, torch_cuda, img, k, aligned_first=False)


def test_enqueue_sep_adversarial(pkg, L, torch_cuda):
    rng = np.random.default_rng(9)
    for c in range(1, 6):
        for (h, w) in ((48, 64), (20, 48), (19, 30)):
            imp = np.zeros((1, h, w, c), np.uint8)
            imp[0, 0, 0] = imp[0, -1, -1] = imp[0, 0, -1] = imp[0, -1, 0] = imp[0, h // 2, w // 2] = 255
            full = np.full((1, h, w, c), 255, np.uint8)
            for r in (1, 7, 16):
                wx, wy = rand_taps(rng, r, 8), rand_taps(rng, max(0, r - 3), 8)
                assert np.array_equal(gpu_sep(pkg, L, torch_cuda, imp, wx, wy), ref_sep(imp, wx, wy)), (c, h, w, r)
                assert np.array_equal(gpu_sep(pkg, L, torch_cuda, full, wx, wy), full)
    img = rng.integers(0, 256, size=(2, 45, 64, 3), dtype=np.uint8)
    assert np.array_equal(gpu_sep(pkg, L, torch_cuda, img, [1], [1]), img)             # identity


def test_binomial_taps_reproduce_the_golden_hashes(pkg, L, O, torch_cuda, golden):
    for e in golden["k3"]:                                   # 8192x8192x3 included
        host = O.lcg_image(e["h"], e["w"], e["c"])[None]
        got = gpu_sep(pkg, L, torch_cuda, host, [1, 2, 1], [1, 2, 1])
        assert f"{L.mi_blur_fnv1a64(got.ctypes.data, got.size):016x}" == e["out_fnv"], e
    for e in golden["k5_unpinned"]:
        host = O.lcg_image(e["h"], e["w"], e["c"])[None]
        assert f"{O.fnv1a64(gpu_sep(pkg, L, torch_cuda, host, [1, 4, 6, 4, 1], [1, 4, 6, 4, 1])):016x}" == e["out_fnv"]
    rng = np.random.default_rng(4)
    for (n, h, w, c) in TILED_SHAPES + GENERIC_SHAPES:
        img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
        for radius, taps in ((1, [1, 2, 1]), (2, [1, 4, 6, 4, 1])):
            d_in = torch_cuda.from_numpy(img).cuda()
            d_out = torch_cuda.zeros_like(d_in)
            pkg.check(L.mi_blur_enqueue(d_in.data_ptr(), d_out.data_ptr(), w, h, c, radius, n, None))
            torch_cuda.cuda.synchronize()
            assert np.array_equal(gpu_sep(pkg, L, torch_cuda, img, taps, taps), d_out.cpu().numpy()), ((n, h, w, c), radius)


def test_batch_over_2gib(pkg, L, torch_cuda):
    """A batch of more than 2^31 bytes: 64-bit image offsets, 32-bit offsets inside an image."""
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, size=(1, 1024, 1024, 3), dtype=np.uint8)
    n = 720                                                   # 2.26 GB in, as much out
    check_batch_over_2gib(SEP, pkg, L, torch_cuda, img, [pkg.gauss_kernel(2.0)], n, same=(0, 1, n // 2, n - 1),
                          patch_last=False, check_kernel=False)


def test_bands_split_with_halo_ry_equal_whole(pkg, L, torch_cuda):
    rng = np.random.default_rng(12)
    for (h, w, c) in ((240, 320, 3), (64, 48, 4), (37, 17, 3)):
        img = rng.integers(0, 256, size=(1, h, w, c), dtype=np.uint8)
        k = pkg.gauss_kernel(1.5, 4.0)
        whole = gpu_run(SEP, pkg, L, torch_cuda, img, k)
        assert np.array_equal(whole, ref_sep(img, *k.taps()))
        check_gpu_band_split_equals_whole(SEP, pkg, L, torch_cuda, img, k, whole, (k.ry, h // 3, h // 2, h - k.ry))


def test_context_with_a_kernel(pkg, L, torch_cuda):
    """Every submit form of a GPU context takes the kernel: pinned (in place, one launch: not the batch server), pageable,
    strided bands, planar."""
    rng = np.random.default_rng(21)
    n, h, w, c = 6, 240, 320, 3                                # 1.38 MB of output per submit: the server size class
    img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    check_gpu_context(SEP, pkg, L, img, pkg.gauss_kernel(2.5, 1.0), pinned_repeats=3)
    # a context without a kernel still takes the batch server for the same pinned submits
    with pkg.Context(0, w, h, c, 1, max_batch=n, n_slots=3) as ctx:
        pin_in, pin_out = L.mi_blur_host_alloc(img.size), L.mi_blur_host_alloc(img.size)
        try:
            np.ctypeslib.as_array((C.c_uint8 * img.size).from_address(pin_in))[:] = img.reshape(-1)
            ctx.submit(pin_in, pin_out, n)
            ctx.sync()
            assert L.mi_blur_last_kernel() == b"blur_server_kernel"
            b = np.ctypeslib.as_array((C.c_uint8 * img.size).from_address(pin_out)).reshape(img.shape)
            assert np.array_equal(b, ref_sep(img, [1, 2, 1], [1, 2, 1]))
        finally:
            L.mi_blur_host_free(pin_in)
            L.mi_blur_host_free(pin_out)


def test_gaussian_blur_python(pkg, torch_cuda):
    rng = np.random.default_rng(30)
    imgs = rng.integers(0, 256, size=(4, 90, 128, 3), dtype=np.uint8)
    for sigma, sy in ((1.0, None), (2.0, None), (5.0, None), (0.7, 3.2)):
        k = pkg.gauss_kernel(sigma, sy)
        assert np.array_equal(pkg.gaussian_blur(imgs, sigma, sy), ref_sep(imgs, *k.taps())), sigma
    g = imgs[0, :, :, 0]
    assert np.array_equal(pkg.gaussian_blur(g, 3.0), ref_sep(g[None, :, :, None], *pkg.gauss_kernel(3.0).taps())[0, :, :, 0])


def test_hosts_sigma_on_the_gpu(pkg, apps, torch_cuda, tmp_path):
    het, spl = apps
    rng = np.random.default_rng(40)
    img = rng.integers(0, 256, size=(240, 320, 3), dtype=np.uint8)
    write_ppm(tmp_path / "in.ppm", img)
    k = pkg.gauss_kernel(2.0)
    want = ref_sep(img[None], *k.taps())[0]
    for cmd, out in (([het, "gpu", "1.0", "35", "--image", "in.ppm", "--images", "100", "--sigma", "2", "--save", "g.ppm"], "g.ppm"),
                     ([het, "both", "0.7", "35", "--image", "in.ppm", "--images", "100", "--sigma", "2", "--save", "b.ppm"], "b.ppm"),
                     ([spl, "0.6", "16", "--image", "in.ppm", "--images", "48", "--sigma", "2", "--save", "s.ppm"], "s.ppm")):
        r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "separable Gaussian, sigma 2 x 2" in r.stdout
        assert np.array_equal(read_ppm(tmp_path / out), want), cmd
    r = subprocess.run([spl, "0.6", "16", "--image", "in.ppm", "--images", "16", "--sigma", "1", "--sigma-y", "5", "--save", "a.ppm"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"Halo size: {pkg.gauss_kernel(1.0, 5.0).ry} row(s)" in r.stdout, r.stdout + r.stderr
    assert np.array_equal(read_ppm(tmp_path / "a.ppm"), ref_sep(img[None], *pkg.gauss_kernel(1.0, 5.0).taps())[0])
