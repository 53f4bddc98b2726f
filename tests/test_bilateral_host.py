"""Bilateral filter (mi_blur_bilateral_gauss, mi_blur_cpu_run_bilateral, mi_blur_ctx_set_bilateral, bilateral_filter(), the
hosts' --bilateral), CPU only: byte for byte against the numpy restatement of the definition in include/mi_blur.h
(bilateral_ref.py), independent of the product.  The filter is defined by integer tables, so every comparison is equality."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import bilateral_ref as br
from bilateral_ref import ref_bilateral
from filter_harness import (BILATERAL, MEDIAN, MORPH, SEP, apps, check_cpu_band_split_equals_whole, check_cpu_context,  # noqa: F401
                            check_set_rules_order, cpu_run, read_ppm, write_ppm)

RADII = tuple(range(1, 9))


def cpu_bilateral(pkg, L, img, k, n_threads=3):
    return cpu_run(BILATERAL, pkg, L, img, k, n_threads)


# ---------------------------------------------------------------- the restatement itself
def test_restatement_against_a_scalar_loop():
    """The vectorised restatement against the definition written out pixel by pixel in Python integers."""
    rng = np.random.default_rng(0)
    for (h, w, c, r) in ((5, 7, 2, 1), (4, 3, 1, 3), (6, 6, 3, 2)):
        img = rng.integers(0, 256, size=(1, h, w, c), dtype=np.uint8)
        S, R = br.random_tables(rng, r, zeros=0.3)
        want = np.zeros_like(img)
        for y in range(h):
            for x in range(w):
                for ch in range(c):
                    v0 = int(img[0, y, x, ch])
                    num = den = 0
                    for j in range(-r, r + 1):
                        for i in range(-r, r + 1):
                            v = int(img[0, min(max(y + j, 0), h - 1), min(max(x + i, 0), w - 1), ch])
                            wgt = int(S[j + r, i + r]) * int(R[abs(v - v0)])
                            den += wgt
                            num += wgt * v
                    want[0, y, x, ch] = (num + den // 2) // den
        assert np.array_equal(ref_bilateral(img, S, R), want), (h, w, c, r)


def test_restatement_timing_shape():
    """4 x 96 x 128 x 3 at radius 8 (289 passes) stays a sub-second reference."""
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(4, 96, 128, 3), dtype=np.uint8)
    S, R = br.gauss_tables(0, 30.0, 8)
    out = ref_bilateral(img, S, R)
    assert out.shape == img.shape and out.dtype == np.uint8


# ---------------------------------------------------------------- mi_blur_bilateral_gauss
def test_gauss_tables_match_the_definition(pkg, L):
    for r in RADII:
        for ss in (0.0, -1.0, 0.3, 0.8, 1.0, 1.7, 2.5, 4.0, 9.0, 50.0):
            for sr in (0.2, 1.0, 3.0, 10.0, 25.0, 60.0, 300.0):
                k = pkg.Bilateral()
                assert L.mi_blur_bilateral_gauss(ss, sr, r, C.byref(k)) == pkg.OK
                S, R = br.gauss_tables(ss, sr, r)
                n = 2 * r + 1
                got_s = np.array(k.spatial[:n * n]).reshape(n, n)
                got_r = np.array(k.range[:])
                assert k.radius == r
                assert np.array_equal(got_s, S), (r, ss, sr)
                assert np.array_equal(got_r, R), (r, ss, sr)
                assert np.array_equal(got_s, got_s.T) and np.array_equal(got_s, got_s[::-1, ::-1])
                assert got_s[r, r] == 128 and got_r[0] == 255
                assert (np.diff(got_r) <= 0).all()
                assert got_s.sum() <= 65535
                assert not any(k.spatial[n * n:])
    k = pkg.Bilateral()
    for ss, sr, r in ((1.0, 0.0, 2), (1.0, -3.0, 2), (1.0, float("nan"), 2), (1.0, 10.0, 0), (1.0, 10.0, 9), (1.0, 10.0, -1)):
        assert L.mi_blur_bilateral_gauss(ss, sr, r, C.byref(k)) == pkg.ERR_INVALID
    assert L.mi_blur_bilateral_gauss(1.0, 10.0, 2, None) == pkg.ERR_INVALID
    g = pkg.Bilateral.gauss(1.5, 20.0, 3)
    S, R = br.gauss_tables(1.5, 20.0, 3)
    assert g.radius == 3 and list(g.spatial[:49]) == S.reshape(-1).tolist() and list(g.range) == R.tolist()


# ---------------------------------------------------------------- mi_blur_cpu_run_bilateral
SHAPES = [(2, 17, 33, 3), (1, 1, 40, 3), (1, 37, 1, 1), (2, 5, 6, 4), (1, 9, 11, 5), (1, 24, 64, 1), (3, 12, 3, 2), (1, 1, 1, 3)]


def test_cpu_run_bilateral_all_radii(pkg, L):
    rng = np.random.default_rng(2)
    for (n, h, w, c) in SHAPES:
        imgs = br.input_kinds(rng, n, h, w, c)
        for r in RADII:
            for tables in (br.gauss_tables(0, 25.0, r), br.random_tables(rng, r), br.random_tables(rng, r, zeros=0.5)):
                k = br.make_kernel(pkg, *tables)
                for q, img in enumerate(imgs[:2] if r > 4 else imgs):
                    want = ref_bilateral(img, *tables)
                    for nt in (1, 4):
                        assert np.array_equal(cpu_bilateral(pkg, L, img, k, nt), want), ((n, h, w, c), r, q, nt)


def test_cpu_run_bilateral_channels_1_to_5(pkg, L):
    rng = np.random.default_rng(3)
    for c in (1, 2, 3, 4, 5):
        img = rng.integers(0, 256, size=(2, 19, 23, c), dtype=np.uint8)
        for r in RADII:
            S, R = br.random_tables(rng, r, zeros=0.2)
            assert np.array_equal(cpu_bilateral(pkg, L, img, br.make_kernel(pkg, S, R)), ref_bilateral(img, S, R)), (c, r)


# ---------------------------------------------------------------- exact properties
def test_exact_properties(pkg, L):
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, size=(2, 21, 26, 3), dtype=np.uint8)
    delta = np.zeros(256, np.int64)
    delta[0] = 255
    ones = np.full(256, 255, np.int64)
    for r in (1, 2, 5, 8):
        n = 2 * r + 1
        S, R = br.random_tables(rng, r)
        # R = [255, 0, 0, ...]: only samples equal to the centre count
        assert np.array_equal(cpu_bilateral(pkg, L, img, br.make_kernel(pkg, S, delta)), img)
        # S with only the centre set
        centre = np.zeros((n, n), np.int64)
        centre[r, r] = 77
        assert np.array_equal(cpu_bilateral(pkg, L, img, br.make_kernel(pkg, centre, R)), img)
        # a constant image stays constant
        for v in (0, 1, 128, 255):
            const = np.full((1, 9, 20, 2), v, np.uint8)
            assert np.array_equal(cpu_bilateral(pkg, L, const, br.make_kernel(pkg, S, R)), const)
        # R all 255: the plain weighted mean, rounded half up
        p = np.pad(img, ((0, 0), (r, r), (r, r), (0, 0)), mode="edge").astype(np.int64)
        acc = np.zeros(img.shape, np.int64)
        for j in range(n):
            for i in range(n):
                acc += int(S[j, i]) * p[:, j:j + 21, i:i + 26, :]
        tot = int(S.sum())
        assert np.array_equal(cpu_bilateral(pkg, L, img, br.make_kernel(pkg, S, ones)), ((acc + tot // 2) // tot).astype(np.uint8))


def test_zero_padded_table_gives_the_same_bytes(pkg, L):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(2, 30, 31, 3), dtype=np.uint8)
    S2, R = br.random_tables(rng, 2)
    S5 = np.zeros((11, 11), np.int64)
    S5[3:8, 3:8] = S2
    a = cpu_bilateral(pkg, L, img, br.make_kernel(pkg, S2, R))
    assert np.array_equal(a, cpu_bilateral(pkg, L, img, br.make_kernel(pkg, S5, R)))
    assert np.array_equal(a, ref_bilateral(img, S2, R))


def test_worst_case_fits_32_bits(pkg, L):
    """289 spatial weights of 128 (sum 36992), R all 255, an image of 255: num is 2 405 404 800 and num + den / 2 stays below 2^32."""
    S = np.full((17, 17), 128, np.int64)
    R = np.full(256, 255, np.int64)
    img = np.full((1, 20, 40, 3), 255, np.uint8)
    assert 289 * 128 * 255 * 255 == 2405404800 and 2405404800 + 289 * 128 * 255 // 2 < 2 ** 32
    assert np.array_equal(cpu_bilateral(pkg, L, img, br.make_kernel(pkg, S, R)), img)
    assert np.array_equal(ref_bilateral(img, S, R), img)
    # the largest spatial sum the validation admits, on the brightest image
    S = np.full((17, 17), 226, np.int64)
    S.reshape(-1)[:65535 - 226 * 289] += 1
    assert S.sum() == 65535
    assert np.array_equal(cpu_bilateral(pkg, L, img, br.make_kernel(pkg, S, R)), img)
    rnd = np.random.default_rng(6).integers(200, 256, size=(1, 20, 40, 3), dtype=np.uint8)
    assert np.array_equal(cpu_bilateral(pkg, L, rnd, br.make_kernel(pkg, S, R)), ref_bilateral(rnd, S, R))


def test_a_step_edge_survives_where_a_blur_smears_it(pkg, L):
    """The filter is not a blur: under a narrow range table a 0/255 step stays 0/255, while the Gaussian blur of the same
    window changes the pixels beside it."""
    img = np.zeros((1, 24, 32, 3), np.uint8)
    img[:, :, 16:] = 255
    for r in (1, 2, 4, 8):
        k = pkg.Bilateral.gauss(0.0, 10.0, r)
        assert np.array_equal(cpu_bilateral(pkg, L, img, k), img), r
        blur = np.empty_like(img)
        g = pkg.gauss_kernel(r / 2.0, radius=r)
        assert L.mi_blur_cpu_run_sep(img.ctypes.data, blur.ctypes.data, 32, 24, 3, 1, C.byref(g), 1) == pkg.OK
        assert not np.array_equal(blur, img), r
        assert 0 < blur[0, 5, 15, 0] < 255 or 0 < blur[0, 5, 16, 0] < 255


def test_division_boundaries(pkg, L):
    """Two-valued windows through every split: quotients on and beside .5."""
    img = br.division_images(40, 48, 2)
    ones = np.full(256, 255, np.int64)
    for r in RADII:
        S = np.ones((2 * r + 1, 2 * r + 1), np.int64)
        assert np.array_equal(cpu_bilateral(pkg, L, img, br.make_kernel(pkg, S, ones)), ref_bilateral(img, S, ones)), r


# ---------------------------------------------------------------- refusals
def test_refusals(pkg, L):
    rng = np.random.default_rng(7)
    a = np.zeros((8, 16, 3), np.uint8)
    b = np.zeros_like(a)
    good = pkg.Bilateral.gauss(0.0, 25.0, 2)
    run = lambda k, i=a.ctypes.data, o=b.ctypes.data, w=16, h=8, c=3, n=1: L.mi_blur_cpu_run_bilateral(i, o, w, h, c, n, k, 1)
    enq = lambda k, i=a.ctypes.data, o=b.ctypes.data, w=16, h=8, c=3, n=1: L.mi_blur_enqueue_bilateral(i, o, w, h, c, n, k, None)
    band = lambda k, i=a.ctypes.data, o=b.ctypes.data, w=16, h=8, c=3: L.mi_blur_enqueue_bilateral_band(i, o, w, h, c, 0, h, k, None)
    assert run(C.byref(good)) == pkg.OK
    bad = []
    for r in (0, 9, -1, 100):
        k = pkg.Bilateral.gauss(0.0, 25.0, 2)
        k.radius = r
        bad.append(k)
    k = pkg.Bilateral.gauss(0.0, 25.0, 2)
    k.spatial[12] = 0                                            # the centre of the 5 x 5
    bad.append(k)
    k = pkg.Bilateral.gauss(0.0, 25.0, 2)
    k.range[0] = 0
    bad.append(k)
    k = br.make_kernel(pkg, np.full((17, 17), 227), np.full(256, 1))   # 227 * 289 = 65603 > 65535
    bad.append(k)
    k = br.make_kernel(pkg, np.full((17, 17), 226), np.full(256, 1))   # 65314: fine
    assert run(C.byref(k)) == pkg.OK
    for k in bad:
        assert run(C.byref(k)) == pkg.ERR_INVALID
        assert enq(C.byref(k)) == pkg.ERR_INVALID                # before MI_BLUR_ERR_NO_DEVICE
        assert band(C.byref(k)) == pkg.ERR_INVALID
    for f in (run, enq, band):
        assert f(None) == pkg.ERR_INVALID
        assert f(C.byref(good), i=None) == pkg.ERR_INVALID
        assert f(C.byref(good), o=None) == pkg.ERR_INVALID
        assert f(C.byref(good), o=a.ctypes.data) == pkg.ERR_INVALID
        assert f(C.byref(good), w=0) == pkg.ERR_INVALID
        assert f(C.byref(good), h=-1) == pkg.ERR_INVALID
        assert f(C.byref(good), c=0) == pkg.ERR_INVALID
    assert run(C.byref(good), n=-1) == pkg.ERR_INVALID and enq(C.byref(good), n=-1) == pkg.ERR_INVALID
    if L.mi_blur_device_count() <= 0:
        assert enq(C.byref(good)) == pkg.ERR_NO_DEVICE           # a valid call without a device: only then NO_DEVICE
    with pytest.raises(ValueError):
        pkg.Bilateral.from_tables([[1, 2], [3, 4]], [1] * 256)
    with pytest.raises(ValueError):
        pkg.Bilateral.from_tables([[1] * 3] * 3, [1] * 255)
    with pytest.raises(ValueError):
        pkg.Bilateral.from_tables([[1] * 3, [1, 256, 1], [1] * 3], [1] * 256)
    with pytest.raises(ValueError):
        pkg.Bilateral.from_tables([[1] * 19] * 19, [1] * 256)
    del rng


# ---------------------------------------------------------------- contexts
def test_cpu_context_with_a_bilateral(pkg, L):
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, size=(3, 40, 24, 3), dtype=np.uint8)

    def spoil(k):                                                # the context keeps a copy
        k.range[0] = 0

    for tables in (br.gauss_tables(0, 25.0, 1), br.random_tables(rng, 3, zeros=0.3), br.gauss_tables(3.0, 40.0, 8)):
        check_cpu_context(BILATERAL, pkg, L, img, br.make_kernel(pkg, *tables), dict(n_threads=2), spoil=spoil)


def test_band_split_with_halo_r_equals_whole(pkg, L):
    rng = np.random.default_rng(12)
    h, w, c = 75, 23, 3
    img = rng.integers(0, 256, size=(1, h, w, c), dtype=np.uint8)
    for r in (1, 4, 8):
        k = br.make_kernel(pkg, *br.random_tables(rng, r, zeros=0.2))
        check_cpu_band_split_equals_whole(BILATERAL, pkg, L, img, k, (r, h // 3, h // 2, h - r), dict(n_threads=2))


def test_set_bilateral_rules(pkg, L):
    """A context holds one filter: set_kernel, set_median, set_morph and set_bilateral each replace what another set."""
    rng = np.random.default_rng(13)
    img = rng.integers(0, 256, size=(2, 20, 24, 3), dtype=np.uint8)
    tables = br.gauss_tables(0, 30.0, 2)
    other = br.random_tables(rng, 4)
    kern, med, mor = (SEP, pkg.gauss_kernel(2.0)), (MEDIAN, 2), (MORPH, (pkg.MORPH_DILATE, 3, 1))
    bil = (BILATERAL, br.make_kernel(pkg, *tables))
    bad_radius, bad_range = br.make_kernel(pkg, *tables), br.make_kernel(pkg, *tables)
    bad_radius.radius = 9
    bad_range.range[0] = 0
    check_set_rules_order(BILATERAL, pkg, L, img,
                          [(kern, bil), (med, bil), (mor, bil), (kern, med, mor, bil), (bil, (BILATERAL, br.make_kernel(pkg, *other))),
                           (bil, med), (bil, kern), (bil, mor)],
                          refused=[bad_radius, bad_range, None], good=bil[1])


# ---------------------------------------------------------------- Python function
def test_bilateral_filter_on_the_cpu_device(pkg):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(40, 50, 3), dtype=np.uint8)
    for k in (3, 5, 9, 17):
        got = pkg.bilateral_filter(img, k, device=pkg.DEVICE_CPU)
        assert got.shape == img.shape and np.array_equal(got, ref_bilateral(img[None], *br.gauss_tables(k / 4.0, 25.0, k // 2))[0]), k
    got = pkg.bilateral_filter(img, 7, sigma_color=60.0, sigma_space=2.5, device=pkg.DEVICE_CPU)
    assert np.array_equal(got, ref_bilateral(img[None], *br.gauss_tables(2.5, 60.0, 3))[0])
    assert np.array_equal(pkg.bilateral_filter(img, device=pkg.DEVICE_CPU), ref_bilateral(img[None], *br.gauss_tables(1.25, 25.0, 2))[0])
    g = img[:, :, 0]
    got = pkg.bilateral_filter(g, 5, device=pkg.DEVICE_CPU)
    assert got.shape == g.shape and np.array_equal(got, ref_bilateral(g[None, :, :, None], *br.gauss_tables(1.25, 25.0, 2))[0, :, :, 0])
    batch = rng.integers(0, 256, size=(3, 12, 10, 4), dtype=np.uint8)
    assert np.array_equal(pkg.bilateral_filter(batch, 3, device=pkg.DEVICE_CPU, batch=2), ref_bilateral(batch, *br.gauss_tables(0.75, 25.0, 1)))
    for bad in (0, 1, 2, 4, 19, -3, (3, 3), 3.0, "3", None, True):
        with pytest.raises(ValueError):
            pkg.bilateral_filter(img, bad, device=pkg.DEVICE_CPU)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError):
            pkg.bilateral_filter(img, 5, sigma_color=bad, device=pkg.DEVICE_CPU)
    with pytest.raises(ValueError):
        pkg.bilateral_filter(img.astype(np.float32), 3, device=pkg.DEVICE_CPU)


# ---------------------------------------------------------------- hosts
def test_host_cpu_bilateral(apps, tmp_path):
    het, _ = apps
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, size=(45, 61, 3)).astype(np.uint8)
    write_ppm(tmp_path / "in.ppm", img)
    for k, extra, sc, ss in ((5, [], 25.0, 1.25), (9, ["--sigma-color", "40"], 40.0, 2.25),
                             (3, ["--sigma-color", "12.5", "--sigma-space", "2"], 12.5, 2.0), (17, ["--sigma-space", "0"], 25.0, 4.25)):
        r = subprocess.run([het, "cpu", "0.5", "7", "--image", "in.ppm", "--images", "20", "--bilateral", str(k)] + extra +
                           ["--save", "out.ppm"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"Blur kernel: {k}x{k} bilateral (sigma_color {sc:g}, sigma_space {ss:g})\n" in r.stdout
        assert np.array_equal(read_ppm(tmp_path / "out.ppm"), ref_bilateral(img[None], *br.gauss_tables(ss, sc, k // 2))[0]), k


def test_host_bilateral_refusals(apps, tmp_path):
    het, spl = apps
    syn = [het, "cpu", "--synthetic"]
    for cmd in (syn + ["--bilateral", "4"], syn + ["--bilateral", "19"], syn + ["--bilateral", "1"], syn + ["--bilateral"],
                syn + ["--bilateral", "5", "--sigma", "2"], syn + ["--ksize", "3", "--bilateral", "5"],
                syn + ["--median", "5", "--bilateral", "5"], syn + ["--bilateral", "5", "--erode", "3"],
                syn + ["--dilate", "3", "--bilateral", "5"], syn + ["--bilateral", "5", "--morph-gradient", "3"],
                syn + ["--bilateral", "5", "--sigma-color", "0"], syn + ["--bilateral", "5", "--sigma-color", "-2"],
                syn + ["--bilateral", "5", "--sigma-space", "-1"], syn + ["--sigma-color", "10"], syn + ["--sigma-space", "2"],
                [het, "gpu", "--bilateral", "3", "--resident"], [spl, "--resident", "--bilateral", "3"],
                [spl, "--synthetic", "--bilateral", "6"]):
        r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Error:" in r.stdout, (cmd, r.stdout)
