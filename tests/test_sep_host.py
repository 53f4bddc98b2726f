"""Separable kernels of any radius (mi_blur_gauss_taps, mi_blur_cpu_run_sep, mi_blur_ctx_set_kernel, the hosts' --sigma),
CPU only: against a numpy restatement of the definition in include/mi_blur.h (sep_ref.py), independent of the product."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from filter_harness import SEP, apps, check_cpu_context, cpu_run, read_ppm, write_ppm  # noqa: F401
from sep_ref import rand_taps, ref_sep, ref_taps


@pytest.fixture(scope="module")
def sep(pkg, L):
    return pkg


def cpu_sep(pkg, L, img, wx, wy, n_threads=3):
    return cpu_run(SEP, pkg, L, img, pkg.SepKernel.from_taps(wx, wy), n_threads)


# ---------------------------------------------------------------- taps
def test_gauss_taps_match_the_definition(sep):
    for bits in range(4, 9):
        for sigma in np.round(np.arange(0.3, 6.01, 0.1), 2):
            for radius in (0, 1, 3, 16):
                want = ref_taps(float(sigma), radius, bits)
                if want is None:
                    with pytest.raises(sep.MiBlurError) as e:
                        sep.gauss_taps(float(sigma), radius, bits)
                    assert e.value.status == sep.ERR_INVALID
                    continue
                got = sep.gauss_taps(float(sigma), radius, bits)
                assert got == want, (sigma, radius, bits)
                assert sum(got) == 1 << bits and len(got) % 2 == 1 and len(got) <= 33
    assert sep.gauss_taps(1.0) == ref_taps(1.0) and len(sep.gauss_taps(1.0)) == 7      # ceil(3 sigma) = 3
    assert len(sep.gauss_taps(12.0)) == 33                                            # clamped to 16
    assert sep.gauss_taps(0.05) == [256]                                              # every outer pair trimmed


def test_gauss_taps_invalid(sep, L):
    taps = (C.c_uint16 * 33)()
    r = C.c_int()
    for args in [(0.0, 0, 8), (-1.0, 0, 8), (float("nan"), 0, 8), (1.0, -1, 8), (1.0, 17, 8), (1.0, 0, 9), (1.0, 0, -1)]:
        assert L.mi_blur_gauss_taps(*args, taps, C.byref(r)) == sep.ERR_INVALID, args
    assert ref_taps(100.0, 1, 1) is None                                              # centre corrected to 0
    assert L.mi_blur_gauss_taps(100.0, 1, 1, taps, C.byref(r)) == sep.ERR_INVALID
    assert L.mi_blur_gauss_taps(1.0, 0, 8, None, C.byref(r)) == sep.ERR_INVALID
    k = sep.SepKernel()
    assert L.mi_blur_sep_kernel_gauss(2.0, 0.0, 0, 8, C.byref(k)) == sep.OK
    assert (k.rx, k.ry, k.bx, k.by) == (6, 6, 8, 8) and k.taps()[0] == ref_taps(2.0)
    assert L.mi_blur_sep_kernel_gauss(1.0, 3.0, 0, 6, C.byref(k)) == sep.OK
    assert k.taps() == (ref_taps(1.0, 0, 6), ref_taps(3.0, 0, 6)) and (k.bx, k.by) == (6, 6)
    assert L.mi_blur_sep_kernel_gauss(1.0, 3.0, 2, 8, C.byref(k)) == sep.OK and (k.rx, k.ry) == (2, 2)
    assert L.mi_blur_sep_kernel_gauss(0.0, 1.0, 0, 8, C.byref(k)) == sep.ERR_INVALID


def test_invalid_kernels_are_refused(sep, L):
    a = np.zeros((8, 8, 3), np.uint8)
    b = np.zeros_like(a)
    good = sep.SepKernel.from_taps([1, 2, 1])
    assert L.mi_blur_cpu_run_sep(a.ctypes.data, b.ctypes.data, 8, 8, 3, 1, C.byref(good), 1) == sep.OK
    bad = []
    k = sep.SepKernel.from_taps([1, 2, 1]); k.wx[0] = 2; bad.append(k)                 # sum 5: not 2^bx
    k = sep.SepKernel.from_taps([1, 2, 1]); k.bx = 3; bad.append(k)                    # sum 4 != 2^3
    k = sep.SepKernel.from_taps([1, 2, 1]); k.rx = 17; bad.append(k)                   # radius > 16
    k = sep.SepKernel.from_taps([1, 2, 1]); k.ry = -1; bad.append(k)
    k = sep.SepKernel.from_taps([512], [1]); bad.append(k)                              # bx = 9
    for k in bad:
        assert L.mi_blur_cpu_run_sep(a.ctypes.data, b.ctypes.data, 8, 8, 3, 1, C.byref(k), 1) == sep.ERR_INVALID
        assert L.mi_blur_enqueue_sep(a.ctypes.data, b.ctypes.data, 8, 8, 3, 1, C.byref(k), None) == sep.ERR_INVALID
    for args in [(a.ctypes.data, a.ctypes.data, 8, 8, 3, 1), (a.ctypes.data, b.ctypes.data, 0, 8, 3, 1),
                 (a.ctypes.data, b.ctypes.data, 8, 8, 0, 1), (a.ctypes.data, b.ctypes.data, 8, 8, 3, -1),
                 (None, b.ctypes.data, 8, 8, 3, 1)]:
        assert L.mi_blur_cpu_run_sep(*args, C.byref(good), 1) == sep.ERR_INVALID, args
    assert L.mi_blur_cpu_run_sep(a.ctypes.data, b.ctypes.data, 8, 8, 3, 1, None, 1) == sep.ERR_INVALID
    with pytest.raises(ValueError):
        sep.SepKernel.from_taps([1, 2])


# ---------------------------------------------------------------- CPU device
SHAPES = [(1, 1, 1, 3), (2, 17, 33, 3), (1, 40, 64, 4), (3, 9, 5, 1), (1, 31, 29, 2), (1, 50, 7, 5), (2, 3, 100, 3)]


def test_cpu_run_sep_random_taps(sep, L):
    rng = np.random.default_rng(7)
    for (n, h, w, c) in SHAPES:
        img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
        for rx, ry in [(0, 3), (4, 0), (2, 5), (16, 16), (1, 16), (0, 0), (7, 2)]:
            wx, wy = rand_taps(rng, rx, int(rng.integers(0, 9))), rand_taps(rng, ry, int(rng.integers(0, 9)))
            assert np.array_equal(cpu_sep(sep, L, img, wx, wy), ref_sep(img, wx, wy)), ((n, h, w, c), wx, wy)


def test_cpu_run_sep_identity_and_extremes(sep, L):
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(2, 23, 19, 3), dtype=np.uint8)
    assert np.array_equal(cpu_sep(sep, L, img, [1], [1]), img)
    full = np.full((1, 20, 20, 3), 255, np.uint8)
    wx = sep.gauss_taps(5.0)
    assert np.array_equal(cpu_sep(sep, L, full, wx, wx), full)
    imp = np.zeros((1, 21, 21, 1), np.uint8)
    imp[0, 0, 0] = imp[0, -1, -1] = imp[0, 10, 10] = 255
    for r in (1, 8, 16):
        wx = rand_taps(rng, r, 8)
        assert np.array_equal(cpu_sep(sep, L, imp, wx, wx[::-1]), ref_sep(imp, wx, wx[::-1]))


def test_binomial_taps_are_the_fixed_kernels(sep, L, O, golden):
    """{1,2,1} through the separable path is the reference 3x3 byte for byte (golden k3 hashes); {1,4,6,4,1} is radius 2."""
    for e in golden["k3"]:
        if e["h"] * e["w"] > 2200 * 2200:
            continue
        img = O.lcg_image(e["h"], e["w"], e["c"])[None]
        out = cpu_sep(sep, L, img, [1, 2, 1], [1, 2, 1])
        assert f"{L.mi_blur_fnv1a64(out.ctypes.data, out.size):016x}" == e["out_fnv"], e
    for e in golden["k5_unpinned"]:
        img = O.lcg_image(e["h"], e["w"], e["c"])[None]
        assert f"{O.fnv1a64(cpu_sep(sep, L, img, [1, 4, 6, 4, 1], [1, 4, 6, 4, 1])):016x}" == e["out_fnv"]
    rng = np.random.default_rng(3)
    for (n, h, w, c) in SHAPES:
        img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
        want = np.empty_like(img)
        pkg_rc = L.mi_blur_cpu_run(img.ctypes.data, want.ctypes.data, w, h, c, 2, n, 2)
        assert pkg_rc == sep.OK
        assert np.array_equal(cpu_sep(sep, L, img, [1, 4, 6, 4, 1], [1, 4, 6, 4, 1]), want)


def test_cpu_context_with_a_kernel(sep, L):
    rng = np.random.default_rng(11)
    n, h, w, c = 5, 37, 41, 3
    img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    # halo rows 3 above and 2 below whatever the kernel's own radius (sigma_y 1: 3)
    check_cpu_context(SEP, sep, L, img, sep.gauss_kernel(2.0, 1.0), dict(n_slots=2, n_threads=3), halos=(3, 2))
    with sep.Context(sep.DEVICE_CPU, w, h, c, 1, max_batch=n) as ctx:
        bad = sep.SepKernel.from_taps([1, 2, 1]); bad.bx = 1
        assert L.mi_blur_ctx_set_kernel(ctx.h, C.byref(bad)) == sep.ERR_INVALID
        assert L.mi_blur_ctx_set_kernel(ctx.h, None) == sep.ERR_INVALID
        out = np.zeros_like(img)                                                            # no kernel: the radius it was made with
        ctx.submit(img.ctypes.data, out.ctypes.data, n)
        ctx.sync()
        assert np.array_equal(out, ref_sep(img, [1, 2, 1], [1, 2, 1]))


def test_gaussian_blur_on_the_cpu_device(sep):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(30, 50, 3), dtype=np.uint8)
    k = sep.gauss_kernel(3.0, 1.5)
    assert np.array_equal(sep.gaussian_blur(img, 3.0, 1.5, device=sep.DEVICE_CPU), ref_sep(img[None], *k.taps())[0])
    g = img[:, :, 0]
    assert np.array_equal(sep.gaussian_blur(g, 1.0, device=sep.DEVICE_CPU), ref_sep(g[None, :, :, None], *sep.gauss_kernel(1.0).taps())[0, :, :, 0])


# ---------------------------------------------------------------- hosts
def test_host_cpu_sigma(sep, apps, tmp_path):
    het, _ = apps
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, size=(45, 61, 3), dtype=np.uint8)
    write_ppm(tmp_path / "in.ppm", img)
    r = subprocess.run([het, "cpu", "0.5", "7", "--image", "in.ppm", "--images", "20", "--sigma", "2", "--save", "out.ppm"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    taps = sep.gauss_taps(2.0)
    assert "Blur kernel: 13x13 separable Gaussian, sigma 2 x 2" in r.stdout
    assert "Taps x (/256): " + " ".join(map(str, taps)) in r.stdout
    assert np.array_equal(read_ppm(tmp_path / "out.ppm"), ref_sep(img[None], taps, taps)[0])
    r = subprocess.run([het, "cpu", "0.5", "7", "--image", "in.ppm", "--images", "7", "--sigma", "1", "--sigma-y", "4",
                        "--radius", "5", "--save", "aniso.ppm"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    k = sep.gauss_kernel(1.0, 4.0, 5)
    assert np.array_equal(read_ppm(tmp_path / "aniso.ppm"), ref_sep(img[None], *k.taps())[0])
    # plain command lines print what they always printed
    r = subprocess.run([het, "cpu", "0.5", "7", "--image", "in.ppm", "--images", "7"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Blur kernel: 3x3\n" in r.stdout and "Taps" not in r.stdout


def test_host_sigma_refusals(apps, tmp_path):
    het, spl = apps
    for cmd in ([het, "cpu", "--synthetic", "--sigma", "2", "--ksize", "5"], [het, "gpu", "--sigma", "2", "--resident"],
                [spl, "--resident", "--sigma", "2"], [het, "cpu", "--radius", "3"], [het, "cpu", "--sigma", "0"],
                [spl, "--sigma", "1", "--radius", "17"]):
        r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Error:" in r.stdout, (cmd, r.stdout)
