"""Signed 2-D convolution (mi_blur_conv_preset, mi_blur_cpu_run_conv, mi_blur_ctx_set_conv, filter2d() / sobel() / scharr() /
laplacian() / sharpen(), the hosts' --conv), CPU only: byte for byte against the numpy restatement of the definition in
include/mi_blur.h (conv_ref.py), independent of the product.  The filter is defined in integers, so every comparison is
equality."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import conv_ref as cr
from conv_ref import ref_conv
from filter_harness import (BILATERAL, CONV, MEDIAN, MORPH, SEP, apps, check_cpu_band_split_equals_whole, check_cpu_context,  # noqa: F401
                            check_set_rules_order, cpu_run, read_ppm, write_ppm)

# every rx and every ry, in a sample of pairs
PAIRS = [(r, r) for r in range(8)] + [(0, 7), (7, 0), (1, 4), (4, 1), (2, 5), (5, 3), (3, 6), (6, 2), (1, 0), (0, 1), (7, 3), (2, 7)]


def cpu_conv(pkg, L, img, k, n_threads=3):
    return cpu_run(CONV, pkg, L, img, k, n_threads)


def run_spec(pkg, L, img, spec, n_threads=3):
    return cpu_conv(pkg, L, img, cr.make_kernel(pkg, **spec), n_threads)


# ---------------------------------------------------------------- the restatement itself
def test_restatement_against_a_scalar_loop():
    """The vectorised restatement against the definition written out pixel by pixel in Python integers."""
    rng = np.random.default_rng(0)
    for (h, w, c, rx, ry, mode) in ((5, 7, 2, 1, 1, "sat"), (4, 3, 1, 3, 0, "abs"), (6, 6, 3, 2, 1, "mag"), (3, 5, 1, 0, 2, "sat")):
        img = rng.integers(0, 256, size=(1, h, w, c), dtype=np.uint8)
        spec = cr.random_kernel(rng, rx, ry, zeros=0.3, mode=mode)
        want = np.zeros_like(img)
        for y in range(h):
            for x in range(w):
                for ch in range(c):
                    acc = acc2 = 0
                    for j in range(-ry, ry + 1):
                        for i in range(-rx, rx + 1):
                            v = int(img[0, min(max(y + j, 0), h - 1), min(max(x + i, 0), w - 1), ch])
                            acc += int(spec["K"][j + ry, i + rx]) * v
                            if mode == "mag":
                                acc2 += int(spec["K2"][j + ry, i + rx]) * v
                    a = acc if mode == "sat" else abs(acc) + abs(acc2)
                    want[0, y, x, ch] = min(max((a + spec["bias"]) // (1 << spec["shift"]), 0), 255)     # // is the floor
        assert np.array_equal(ref_conv(img, **spec), want), (h, w, c, rx, ry, mode)


# ---------------------------------------------------------------- mi_blur_cpu_run_conv
SHAPES = [(2, 17, 33, 3), (1, 1, 40, 3), (1, 37, 1, 1), (2, 5, 6, 4), (1, 24, 64, 1), (1, 1, 1, 3)]


def test_cpu_run_conv_radius_pairs_and_modes(pkg, L):
    rng = np.random.default_rng(2)
    assert {p[0] for p in PAIRS} == set(range(8)) and {p[1] for p in PAIRS} == set(range(8))
    for (n, h, w, c) in SHAPES:
        imgs = cr.input_kinds(rng, n, h, w, c)
        for q, (rx, ry) in enumerate(PAIRS):
            for mode in cr.MODES:
                spec = cr.random_kernel(rng, rx, ry, zeros=(0.0, 0.4)[q % 2], mode=mode)
                k = cr.make_kernel(pkg, **spec)
                for z, img in enumerate(imgs[:2] if q % 3 else imgs):
                    want = ref_conv(img, **spec)
                    for nt in (1, 4):
                        assert np.array_equal(cpu_conv(pkg, L, img, k, nt), want), ((n, h, w, c), rx, ry, mode, z, nt)


def test_cpu_run_conv_channels_1_to_5(pkg, L):
    rng = np.random.default_rng(3)
    for c in (1, 2, 3, 4, 5):
        img = rng.integers(0, 256, size=(2, 19, 23, c), dtype=np.uint8)
        for (rx, ry) in PAIRS[:12]:
            for mode in cr.MODES:
                spec = cr.random_kernel(rng, rx, ry, zeros=0.2, mode=mode)
                assert np.array_equal(run_spec(pkg, L, img, spec), ref_conv(img, **spec)), (c, rx, ry, mode)


def test_orientation_is_correlation(pkg, L):
    """A single tap at (j = -1, i = +2): the output is the image one row up and two columns to the right, clamped."""
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, size=(2, 9, 11, 3), dtype=np.uint8)
    K = np.zeros((3, 5), np.int64)
    K[-1 + 1, 2 + 2] = 1
    yy = np.clip(np.arange(9) - 1, 0, 8)
    xx = np.clip(np.arange(11) + 2, 0, 10)
    want = img[:, yy][:, :, xx]
    assert np.array_equal(run_spec(pkg, L, img, dict(K=K)), want)
    assert np.array_equal(ref_conv(img, K), want)
    assert not np.array_equal(run_spec(pkg, L, img, dict(K=K[::-1, ::-1])), want)


# ---------------------------------------------------------------- anchors to existing ground truth
def test_binomial_kernels_equal_the_box_blurs_and_the_golden_vectors(pkg, L, O, golden):
    b3, b5 = np.array([1, 2, 1]), np.array([1, 4, 6, 4, 1])
    k3 = cr.make_kernel(pkg, np.outer(b3, b3), shift=4)
    k5 = cr.make_kernel(pkg, np.outer(b5, b5), shift=8)
    rng = np.random.default_rng(5)
    for img in (O.lcg_stream(2, 33, 40, 3), rng.integers(0, 256, size=(1, 17, 16, 4), dtype=np.uint8), rng.integers(0, 256, size=(1, 5, 7, 5), dtype=np.uint8)):
        assert np.array_equal(cpu_conv(pkg, L, img, k3), O.blur_batch(img, 1))
        assert np.array_equal(cpu_conv(pkg, L, img, k5), O.blur_batch(img, 2))
        box = np.empty_like(img)
        n, h, w, c = img.shape
        pkg.check(L.mi_blur_cpu_run(img.ctypes.data, box.ctypes.data, w, h, c, 2, n, 1))
        assert np.array_equal(cpu_conv(pkg, L, img, k5), box)
    checked = 0
    for e in golden["k3"]:
        if e["h"] * e["w"] > 2200 * 2200:
            continue
        img = O.lcg_image(e["h"], e["w"], e["c"])
        out = cpu_conv(pkg, L, img[None], k3)[0]
        assert out.reshape(-1)[:8].tolist() == e["first"][:out.size]
        assert f"{O.fnv1a64(out):016x}" == e["out_fnv"], e
        checked += 1
    assert checked >= 3


def test_outer_product_of_gauss_taps_equals_the_separable_run(pkg, L):
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, size=(2, 31, 29, 3), dtype=np.uint8)
    n, h, w, c = img.shape
    for sigma in (0.6, 1.0, 1.7, 2.2):
        taps = (C.c_uint16 * 33)()
        r = C.c_int()
        assert L.mi_blur_gauss_taps(sigma, 0, 6, taps, C.byref(r)) == pkg.OK
        t = np.array(taps[:2 * r.value + 1], np.int64)
        assert r.value <= 7 and t.sum() == 64
        sep = pkg.SepKernel.from_taps(t.tolist())
        want = np.empty_like(img)
        pkg.check(L.mi_blur_cpu_run_sep(img.ctypes.data, want.ctypes.data, w, h, c, n, C.byref(sep), 1))
        assert np.array_equal(run_spec(pkg, L, img, dict(K=np.outer(t, t), shift=12)), want), sigma


def test_all_ones_is_the_window_sum(pkg, L):
    rng = np.random.default_rng(7)
    img = rng.integers(0, 29, size=(1, 12, 14, 2), dtype=np.uint8)           # 9 * 28 = 252: no saturation
    p = np.pad(img, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge").astype(np.int64)
    want = sum(p[:, j:j + 12, i:i + 14] for j in range(3) for i in range(3))
    assert want.max() <= 255
    assert np.array_equal(run_spec(pkg, L, img, dict(K=np.ones((3, 3), np.int64))), want.astype(np.uint8))


# ---------------------------------------------------------------- presets
SOBEL_X = [[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]]
SCHARR_X = [[-3, 0, 3], [-10, 0, 10], [-3, 0, 3]]
T = lambda k: np.array(k).T.tolist()
PRESETS = {  # name: (id, K, K2, mode, shift, bias)
    "sobel_x": (0, SOBEL_X, None, "abs", 0, 0), "sobel_y": (1, T(SOBEL_X), None, "abs", 0, 0), "sobel_mag": (2, SOBEL_X, T(SOBEL_X), "mag", 0, 0),
    "scharr_x": (3, SCHARR_X, None, "abs", 0, 0), "scharr_y": (4, T(SCHARR_X), None, "abs", 0, 0), "scharr_mag": (5, SCHARR_X, T(SCHARR_X), "mag", 0, 0),
    "laplacian4": (6, [[0, 1, 0], [1, -4, 1], [0, 1, 0]], None, "abs", 0, 0), "laplacian8": (7, [[1, 1, 1], [1, -8, 1], [1, 1, 1]], None, "abs", 0, 0),
    "sharpen": (8, [[0, -1, 0], [-1, 5, -1], [0, -1, 0]], None, "sat", 0, 0), "emboss": (9, [[-2, -1, 0], [-1, 1, 1], [0, 1, 2]], None, "sat", 0, 128)}


def test_presets(pkg, L):
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, size=(2, 20, 21, 3), dtype=np.uint8)
    assert set(pkg.CONV_PRESETS) == set(PRESETS)
    for name, (pid, K, K2, mode, shift, bias) in PRESETS.items():
        k = pkg.Conv()
        C.memset(C.byref(k), 0x7F, C.sizeof(k))
        assert L.mi_blur_conv_preset(pid, C.byref(k)) == pkg.OK and pkg.CONV_PRESETS[name] == pid
        assert (k.rx, k.ry, k.mode, k.shift, k.bias) == (1, 1, pkg.CONV_MODES[mode], shift, bias), name
        assert list(k.k[:9]) == [v for row in K for v in row], name
        assert list(k.k2[:9]) == ([v for row in K2 for v in row] if K2 else [0] * 9), name
        assert not any(k.k[9:]) and not any(k.k2[9:])
        assert np.array_equal(cpu_conv(pkg, L, img, k), ref_conv(img, K, shift, bias, mode, K2)), name
        assert pkg.Conv.preset(name).taps() == (K, K2)
    k = pkg.Conv()
    for bad in (-1, 10, 100):
        assert L.mi_blur_conv_preset(bad, C.byref(k)) == pkg.ERR_INVALID
    assert L.mi_blur_conv_preset(0, None) == pkg.ERR_INVALID
    with pytest.raises(ValueError):
        pkg.Conv.preset("sobel")


def test_sobel_mag_is_the_sum_of_both_gradients(pkg, L):
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, size=(2, 23, 19, 3), dtype=np.uint8)
    p = np.pad(img, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge").astype(np.int64)
    win = lambda j, i: p[:, 1 + j:24 + j, 1 + i:20 + i]
    gx = (win(-1, 1) + 2 * win(0, 1) + win(1, 1)) - (win(-1, -1) + 2 * win(0, -1) + win(1, -1))
    gy = (win(1, -1) + 2 * win(1, 0) + win(1, 1)) - (win(-1, -1) + 2 * win(-1, 0) + win(-1, 1))
    assert np.array_equal(cpu_conv(pkg, L, img, pkg.Conv.preset("sobel_mag")), np.minimum(255, np.abs(gx) + np.abs(gy)).astype(np.uint8))
    assert np.array_equal(cpu_conv(pkg, L, img, pkg.Conv.preset("sobel_x")), np.minimum(255, np.abs(gx)).astype(np.uint8))
    assert np.array_equal(cpu_conv(pkg, L, img, pkg.Conv.preset("sobel_y")), np.minimum(255, np.abs(gy)).astype(np.uint8))


# ---------------------------------------------------------------- saturation, floor, padding, zeros
def test_saturation_and_floor(pkg, L):
    for c, (h, w) in ((1, (20, 32)), (3, (17, 19))):
        for q, (img, spec) in enumerate(cr.saturation_cases(h, w, c)):
            assert np.array_equal(run_spec(pkg, L, img, spec), ref_conv(img, **spec)), (c, q, spec["mode"], spec["shift"], spec["bias"])
    # negative acc + bias with a shift floors towards minus infinity, then clamps to 0
    img = np.full((1, 4, 5, 1), 9, np.uint8)
    for shift in (1, 3, 8, 16):
        for bias in (0, 8, -1, 1):
            assert not run_spec(pkg, L, img, dict(K=[[-1]], shift=shift, bias=bias)).any()
    assert run_spec(pkg, L, img, dict(K=[[-1]], shift=3, bias=17))[0, 0, 0, 0] == 1     # (17 - 9) >> 3
    assert run_spec(pkg, L, img, dict(K=[[-1]], shift=3, bias=16))[0, 0, 0, 0] == 0     # 7 >> 3
    assert run_spec(pkg, L, img, dict(K=[[-1]], shift=3, bias=1, mode="abs"))[0, 0, 0, 0] == 1   # (9 + 1) >> 3


def test_zero_padded_kernel_gives_the_same_bytes(pkg, L):
    rng = np.random.default_rng(10)
    img = rng.integers(0, 256, size=(2, 30, 31, 3), dtype=np.uint8)
    for mode in cr.MODES:
        spec = cr.random_kernel(rng, 2, 1, mode=mode)
        a = run_spec(pkg, L, img, spec)
        assert np.array_equal(a, ref_conv(img, **spec))
        for (rx, ry) in ((2, 1), (3, 1), (2, 4), (5, 6), (7, 7)):
            big = dict(spec)
            for t in ("K", "K2"):
                if spec[t] is not None:
                    big[t] = np.zeros((2 * ry + 1, 2 * rx + 1), np.int64)
                    big[t][ry - 1:ry + 2, rx - 2:rx + 3] = spec[t]
            assert np.array_equal(run_spec(pkg, L, img, big), a), (mode, rx, ry)


def test_all_zero_kernel_gives_the_constant(pkg, L):
    img = np.random.default_rng(11).integers(0, 256, size=(1, 8, 9, 3), dtype=np.uint8)
    for (rx, ry) in ((0, 0), (1, 1), (7, 7), (3, 0)):
        Z = np.zeros((2 * ry + 1, 2 * rx + 1), np.int64)
        for mode in cr.MODES:
            for shift, bias in ((0, 0), (0, 77), (0, 300), (0, -5), (4, 2047), (16, 2 ** 24), (3, -1)):
                got = run_spec(pkg, L, img, dict(K=Z, shift=shift, bias=bias, mode=mode, K2=Z if mode == "mag" else None))
                assert (got == min(max(bias >> shift, 0), 255)).all(), (rx, ry, mode, shift, bias)


# ---------------------------------------------------------------- refusals
def test_refusals(pkg, L):
    a = np.zeros((8, 16, 3), np.uint8)
    b = np.zeros_like(a)
    good = pkg.Conv.preset("sobel_mag")
    run = lambda k, i=a.ctypes.data, o=b.ctypes.data, w=16, h=8, c=3, n=1: L.mi_blur_cpu_run_conv(i, o, w, h, c, n, k, 1)
    enq = lambda k, i=a.ctypes.data, o=b.ctypes.data, w=16, h=8, c=3, n=1: L.mi_blur_enqueue_conv(i, o, w, h, c, n, k, None)
    band = lambda k, i=a.ctypes.data, o=b.ctypes.data, w=16, h=8, c=3, y0=0, y1=8: L.mi_blur_enqueue_conv_band(i, o, w, h, c, y0, y1, k, None)
    assert run(C.byref(good)) == pkg.OK
    bad = []
    for field, values in (("rx", (-1, 8, 100)), ("ry", (-1, 8)), ("mode", (-1, 3, 7)), ("shift", (-1, 17, 32)), ("bias", (2 ** 24 + 1, -2 ** 24 - 1))):
        for v in values:
            k = pkg.Conv.preset("sobel_x")
            setattr(k, field, v)
            bad.append(k)
    full = np.full((15, 15), 291, np.int64)
    full.reshape(-1)[:65535 - 291 * 225] += 1
    assert run(C.byref(cr.make_kernel(pkg, full))) == pkg.OK and run(C.byref(cr.make_kernel(pkg, -full))) == pkg.OK
    over = full.copy()
    over[7, 7] += 1                                                  # sum |K| = 65536
    bad.append(cr.make_kernel(pkg, over))
    bad.append(cr.make_kernel(pkg, -over))
    bad.append(cr.make_kernel(pkg, full, mode="mag", K2=-over))      # the second table is checked in MAG ...
    k = cr.make_kernel(pkg, full, mode="mag", K2=-over)
    k.mode = pkg.CONV_ABS                                            # ... and ignored otherwise
    assert run(C.byref(k)) == pkg.OK
    for k in (pkg.Conv.preset("sobel_x"),):                          # the bounds themselves are valid
        k.shift, k.bias = 16, 2 ** 24
        assert run(C.byref(k)) == pkg.OK
        k.shift, k.bias = 0, -2 ** 24
        assert run(C.byref(k)) == pkg.OK
    for k in bad:
        assert run(C.byref(k)) == pkg.ERR_INVALID
        assert enq(C.byref(k)) == pkg.ERR_INVALID                    # before MI_BLUR_ERR_NO_DEVICE
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
    for y0, y1 in ((6, 2), (0, 9), (-1, 4), (3, 3)):
        assert band(C.byref(good), y0=y0, y1=y1) == pkg.ERR_INVALID
    if L.mi_blur_device_count() <= 0:
        assert enq(C.byref(good)) == pkg.ERR_NO_DEVICE               # a valid call without a device: only then NO_DEVICE
        assert band(C.byref(good)) == pkg.ERR_NO_DEVICE
    for args in (([[1, 2], [3, 4]],), ([[1] * 17],), ([[1] * 3] * 3, 0, 0, "mag"), ([[1] * 3] * 3, 0, 0, "sat", [[1] * 3] * 3), ([[1] * 3] * 3, 0, 0, "max"),
                 ([[1] * 3] * 3, 0, 0, "mag", [[1] * 5] * 3), ([[1, 40000, 1]],), ([[1.5]],), ([[1, 2, 3], [1, 2]],)):
        with pytest.raises(ValueError):
            pkg.Conv.from_taps(*args)


# ---------------------------------------------------------------- contexts
def test_cpu_context_with_a_conv(pkg, L):
    rng = np.random.default_rng(12)
    img = rng.integers(0, 256, size=(3, 40, 24, 3), dtype=np.uint8)

    def spoil(k):                                                    # the context keeps a copy
        k.shift = 99

    for spec in (dict(K=SOBEL_X, mode="mag", K2=T(SOBEL_X)), cr.random_kernel(rng, 3, 2, zeros=0.3, mode="sat"), cr.random_kernel(rng, 1, 7, mode="abs")):
        check_cpu_context(CONV, pkg, L, img, cr.make_kernel(pkg, **spec), dict(n_threads=2), spoil=spoil)


def test_band_split_with_halo_ry_equals_whole(pkg, L):
    rng = np.random.default_rng(13)
    h, w, c = 75, 23, 3
    img = rng.integers(0, 256, size=(1, h, w, c), dtype=np.uint8)
    for (rx, ry, mode) in ((1, 1, "mag"), (5, 4, "sat"), (2, 7, "abs")):
        k = cr.make_kernel(pkg, **cr.random_kernel(rng, rx, ry, zeros=0.2, mode=mode))
        check_cpu_band_split_equals_whole(CONV, pkg, L, img, k, (ry, h // 3, h // 2, h - ry), dict(n_threads=2))


def test_set_conv_rules(pkg, L):
    """A context holds one filter: set_kernel, set_median, set_morph, set_bilateral and set_conv each replace what another set."""
    rng = np.random.default_rng(14)
    img = rng.integers(0, 256, size=(2, 20, 24, 3), dtype=np.uint8)
    spec = cr.random_kernel(rng, 2, 1, mode="mag")
    other = cr.random_kernel(rng, 4, 3, mode="sat")
    kern, med, mor = (SEP, pkg.gauss_kernel(2.0)), (MEDIAN, 2), (MORPH, (pkg.MORPH_DILATE, 3, 1))
    bil, conv = (BILATERAL, pkg.Bilateral.gauss(0.0, 30.0, 2)), (CONV, cr.make_kernel(pkg, **spec))
    bad_rx, bad_shift = cr.make_kernel(pkg, **spec), cr.make_kernel(pkg, **spec)
    bad_rx.rx = 8
    bad_shift.shift = 17
    check_set_rules_order(CONV, pkg, L, img,
                          [(kern, conv), (med, conv), (mor, conv), (bil, conv), (kern, med, mor, bil, conv),
                           (conv, (CONV, cr.make_kernel(pkg, **other))), (conv, med), (conv, kern), (conv, mor), (conv, bil)],
                          refused=[bad_rx, bad_shift, None], good=conv[1])


# ---------------------------------------------------------------- Python functions
def test_python_functions_on_the_cpu_device(pkg):
    rng = np.random.default_rng(15)
    img = rng.integers(0, 256, size=(40, 50, 3), dtype=np.uint8)
    cpu = pkg.DEVICE_CPU
    ref = lambda name: ref_conv(img[None], PRESETS[name][1], PRESETS[name][4], PRESETS[name][5], PRESETS[name][3], PRESETS[name][2])[0]
    for axis in ("x", "y", "mag"):
        got = pkg.sobel(img, axis, device=cpu)
        assert got.shape == img.shape and np.array_equal(got, ref(f"sobel_{axis}"))
        assert np.array_equal(pkg.scharr(img, axis, device=cpu), ref(f"scharr_{axis}"))
    assert np.array_equal(pkg.sobel(img, device=cpu), ref("sobel_mag"))
    assert np.array_equal(pkg.laplacian(img, device=cpu), ref("laplacian4"))
    assert np.array_equal(pkg.laplacian(img, 8, device=cpu), ref("laplacian8"))
    assert np.array_equal(pkg.sharpen(img, device=cpu), ref("sharpen"))
    spec = cr.random_kernel(rng, 3, 2, mode="mag")
    got = pkg.filter2d(img, spec["K"], spec["shift"], spec["bias"], "mag", spec["K2"], device=cpu)
    assert np.array_equal(got, ref_conv(img[None], **spec)[0])
    emboss = PRESETS["emboss"]
    assert np.array_equal(pkg.filter2d(img, emboss[1], bias=128, device=cpu), ref("emboss"))
    g = img[:, :, 0]                                                 # 2-D greyscale input keeps its shape
    got = pkg.sobel(g, device=cpu)
    assert got.shape == g.shape and np.array_equal(got, ref_conv(g[None, :, :, None], SOBEL_X, mode="mag", K2=T(SOBEL_X))[0, :, :, 0])
    got = pkg.filter2d(g, [[1, 2, 1]], shift=2, device=cpu)
    assert got.shape == g.shape and np.array_equal(got, ref_conv(g[None, :, :, None], [[1, 2, 1]], 2)[0, :, :, 0])
    batch = rng.integers(0, 256, size=(3, 12, 10, 4), dtype=np.uint8)
    assert np.array_equal(pkg.sharpen(batch, device=cpu, batch=2), ref_conv(batch, PRESETS["sharpen"][1]))
    for bad in ("z", "magnitude", 0, None):
        with pytest.raises(ValueError):
            pkg.sobel(img, bad, device=cpu)
    for bad in (0, 6, "4"):
        with pytest.raises(ValueError):
            pkg.laplacian(img, bad, device=cpu)
    with pytest.raises(ValueError):
        pkg.filter2d(img, [[1, 2]], device=cpu)
    with pytest.raises(ValueError):
        pkg.sharpen(img.astype(np.float32), device=cpu)
    with pytest.raises(pkg.MiBlurError):
        pkg.filter2d(img, [[40000 // 2] * 5], device=cpu)             # sum |K| > 65535: refused by the library


# ---------------------------------------------------------------- hosts
HOST_NAMES = {"sobel-x": "sobel_x", "sobel-y": "sobel_y", "sobel": "sobel_mag", "scharr-x": "scharr_x", "scharr-y": "scharr_y", "scharr": "scharr_mag",
              "laplacian": "laplacian4", "laplacian8": "laplacian8", "sharpen": "sharpen", "emboss": "emboss"}


def test_host_cpu_conv(apps, tmp_path):
    het, _ = apps
    rng = np.random.default_rng(16)
    img = rng.integers(0, 256, size=(45, 61, 3)).astype(np.uint8)
    write_ppm(tmp_path / "in.ppm", img)
    for name, preset in HOST_NAMES.items():
        r = subprocess.run([het, "cpu", "0.5", "7", "--image", "in.ppm", "--images", "20", "--conv", name, "--save", "out.ppm"],
                           cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"Blur kernel: 3x3 convolution ({name})\n" in r.stdout
        _, K, K2, mode, shift, bias = PRESETS[preset]
        assert np.array_equal(read_ppm(tmp_path / "out.ppm"), ref_conv(img[None], K, shift, bias, mode, K2)[0]), name


def test_host_conv_refusals(apps, tmp_path):
    het, spl = apps
    syn = [het, "cpu", "--synthetic"]
    for cmd in (syn + ["--conv", "sobel-z"], syn + ["--conv", "SOBEL"], syn + ["--conv", "3"], syn + ["--conv"],
                syn + ["--conv", "sobel", "--sigma", "2"], syn + ["--ksize", "3", "--conv", "sobel"],
                syn + ["--median", "5", "--conv", "sharpen"], syn + ["--conv", "emboss", "--erode", "3"],
                syn + ["--dilate", "3", "--conv", "scharr"], syn + ["--conv", "laplacian", "--morph-gradient", "3"],
                syn + ["--conv", "laplacian8", "--bilateral", "5"], syn + ["--bilateral", "5", "--conv", "sobel-x"],
                [het, "gpu", "--conv", "sobel", "--resident"], [spl, "--resident", "--conv", "sobel"],
                [spl, "--synthetic", "--conv", "edges"]):
        r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Error:" in r.stdout, (cmd, r.stdout)
        assert r.returncode in (255, -1), (cmd, r.returncode)                 # exit(-1)
