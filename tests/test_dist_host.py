"""The distance transform without a GPU (mi_blur_dist_value, mi_blur_cpu_run_dist, mi_blur_cpu_run_dist_u8, the blocking
exports on the CPU device, distance_transform() and its kin): the byte rule at every rounding boundary, the CPU device
against the brute-force definition and the separable restatement of dist_ref.py and against scipy, the named cases, the
extremes, the properties the header names, the statuses, the constants dist_ref.py copies and the sanitizer program."""
import ctypes as C
import os

import numpy as np
import pytest

import dist_ref as R
from resample_harness import needs_gxx, run_sanitized

ONES = 0xFFFFFFFF
LIMITS = (0, 1, 5, 300)


def cpu_table(pkg, L, img, metric, nonzero=0, limit=0, n_threads=3, guard=16):
    """mi_blur_cpu_run_dist into a table of 0xA5A5A5A5 words with `guard` words either side."""
    a = np.ascontiguousarray(img)
    n, h, w, c = a.shape
    buf = np.full(a.size + 2 * guard, 0xA5A5A5A5, np.uint32)
    k = pkg.Dist(metric, nonzero, limit, 0, 0)
    pkg.check(L.mi_blur_cpu_run_dist(a.ctypes.data, buf.ctypes.data + 4 * guard, w, h, c, n, C.byref(k), n_threads), "mi_blur_cpu_run_dist")
    assert (buf[:guard] == 0xA5A5A5A5).all() and (buf[guard + a.size:] == 0xA5A5A5A5).all(), "wrote outside the table"
    return buf[guard:guard + a.size].reshape(a.shape)


def cpu_bytes(pkg, L, img, k, n_threads=3, guard=64):
    """mi_blur_cpu_run_dist_u8 into a buffer of 0xA5 with `guard` bytes either side of the output."""
    a = np.ascontiguousarray(img)
    n, h, w, c = a.shape
    buf = np.full(a.size + 2 * guard, 0xA5, np.uint8)
    pkg.check(L.mi_blur_cpu_run_dist_u8(a.ctypes.data, buf.ctypes.data + guard, w, h, c, n, C.byref(k), n_threads), "mi_blur_cpu_run_dist_u8")
    assert (buf[:guard] == 0xA5).all() and (buf[guard + a.size:] == 0xA5).all(), "wrote outside the output"
    return buf[guard:guard + a.size].reshape(a.shape)


def random_sites(rng, shape, density):
    """Bytes whose zeros are the sites: about `density` of the pixels (0: none at all, 1: all of them)."""
    img = rng.integers(1, 256, size=shape, dtype=np.uint8)
    img[rng.random(shape) < density] = 0
    return img


def one_site(shape, sites):
    """255 everywhere, 0 at every (i, y, x, c) of `sites`."""
    img = np.full(shape, 255, np.uint8)
    for s in sites:
        img[s] = 0
    return img


# ---------------------------------------------------------------- the byte rule, one value at a time
def test_value_l2_at_every_rounding_boundary(pkg, L):
    """For every s in 1..255 the smallest T that gives s is ((2 s - 1)^2 + 3) / 4 (the square is 1 modulo 4), and the value
    one below it gives s - 1; T = 0, NONE, the first T that saturates, and the limit boundary either side."""
    call = L.mi_blur_dist_value
    k = C.byref(pkg.Dist(R.L2, 0, 0, R.BYTE, 0))
    for s in range(1, 256):
        first = ((2 * s - 1) ** 2 + 3) // 4
        assert R.ref_value(R.L2, R.BYTE, 0, first) == s and R.ref_value(R.L2, R.BYTE, 0, first - 1) == s - 1
        assert call(k, first) == s and call(k, first - 1) == s - 1, s
    assert all(R.root_half_up(t) == int(np.floor(np.sqrt(t) + 0.5)) for t in range(0, 70000, 7))
    ts = np.concatenate([np.arange(70000, dtype=np.uint32), np.array([2 ** 31 - 1, top_l2 := 2 * 32767 ** 2, R.NONE], np.uint32)])
    assert R.ref_bytes(ts, R.L2).tolist() == [R.ref_value(R.L2, R.BYTE, 0, t) for t in ts.tolist()] and top_l2 < 2 ** 31
    assert call(k, 0) == 0 and call(k, R.NONE) == 255
    assert ((2 * 255 - 1) ** 2 + 3) // 4 == 64771 and call(k, 64770) == 254 and call(k, 64771) == 255
    top = 2 * 32767 ** 2
    assert call(k, top) == 255 and call(k, top + 1) == -1 and call(k, R.NONE - 1) == -1
    k5 = C.byref(pkg.Dist(R.L2, 1, 5, R.BYTE, 0))
    assert call(k5, 25) == 5 and call(k5, 26) == -1 and call(k5, R.NONE) == 255 and call(k5, 24) == 5 and call(k5, 20) == 4
    for invert in (0, 1):
        w5 = C.byref(pkg.Dist(R.L2, 0, 5, R.WITHIN, invert))
        assert call(w5, 25) == (0 if invert else 255) and call(w5, 0) == (0 if invert else 255)
        assert call(w5, R.NONE) == (255 if invert else 0) and call(w5, 26) == -1


def test_value_l1_and_linf_saturate(pkg, L):
    call = L.mi_blur_dist_value
    for metric, top in ((R.L1, 2 * 32767), (R.LINF, 32767)):
        k = C.byref(pkg.Dist(metric, 0, 0, R.BYTE, 0))
        assert [call(k, t) for t in (0, 1, 254, 255, 256, top)] == [0, 1, 254, 255, 255, 255]
        assert [R.ref_value(metric, R.BYTE, 0, t) for t in (0, 1, 254, 255, 256, top)] == [0, 1, 254, 255, 255, 255]
        assert call(k, top + 1) == -1 and call(k, R.NONE) == 255
        k300 = C.byref(pkg.Dist(metric, 0, 300, R.BYTE, 0))
        assert call(k300, 300) == 255 and call(k300, 301) == -1 and call(k300, 254) == 254
        w = C.byref(pkg.Dist(metric, 0, 300, R.WITHIN, 0))
        assert call(w, 300) == 255 and call(w, 301) == -1 and call(w, R.NONE) == 0


def bad_structs(pkg, bytes_form):
    """Every struct the header calls invalid for the byte calls (bytes_form) or the table calls."""
    D = pkg.Dist
    bad = [D(3, 0, 0, 0, 0), D(-1, 0, 0, 0, 0), D(R.L2, 2, 0, 0, 0), D(R.L2, -1, 0, 0, 0), D(R.L1, 0, -1, 0, 0), D(R.L1, 0, 32768, 0, 0),
           D(R.L2, 0, 0, 2, 0), D(R.L2, 0, 0, -1, 0), D(R.L2, 0, 0, R.BYTE, 1), D(R.LINF, 0, 0, R.WITHIN, 0), D(R.LINF, 0, 3, R.WITHIN, 2),
           D(R.LINF, 0, 3, R.WITHIN, -1)]
    if not bytes_form:
        bad += [D(R.L2, 0, 3, R.WITHIN, 0), D(R.L2, 0, 3, R.WITHIN, 1)]
    return bad


def test_value_refuses_every_invalid_struct(pkg, L):
    for k in bad_structs(pkg, True):
        assert L.mi_blur_dist_value(C.byref(k), 0) == -1, (k.metric, k.sites_nonzero, k.limit, k.byte_op, k.invert)
    assert L.mi_blur_dist_value(None, 0) == -1


# ---------------------------------------------------------------- the CPU device against the definition
@pytest.mark.parametrize("metric", R.METRICS)
def test_cpu_device_equals_the_brute_force_definition(pkg, L, metric):
    """Both site conventions, limits 0, 1, 5 and 300, densities 0, 2 %, 20 % and 1, random shapes up to 40 x 40 x C."""
    rng = np.random.default_rng(100 + metric)
    for density in (0.0, 0.02, 0.2, 1.0):
        for rep in range(3):
            shape = (int(rng.integers(1, 3)), int(rng.integers(1, 41)), int(rng.integers(1, 41)), int(rng.integers(1, 5)))
            img = random_sites(rng, shape, density)
            for nonzero in (0, 1):
                for limit in LIMITS:
                    want = R.ref_brute(img, metric, nonzero, limit)
                    got = cpu_table(pkg, L, img, metric, nonzero, limit, n_threads=1 + rep)
                    assert np.array_equal(got, want), (shape, density, nonzero, limit)
                    if limit in (0, 5):
                        for k in (pkg.Dist(metric, nonzero, limit, R.BYTE, 0),) + ((pkg.Dist(metric, nonzero, limit, R.WITHIN, rep & 1),) if limit else ()):
                            assert np.array_equal(cpu_bytes(pkg, L, img, k), R.ref_bytes(want, metric, k.byte_op, k.invert)), (shape, limit, k.byte_op)


def test_the_two_restatements_agree(pkg):
    rng = np.random.default_rng(7)
    for shape in ((2, 9, 13, 3), (1, 20, 33, 1), (1, 1, 40, 2)):
        for density in (0.0, 0.05, 0.5):
            img = random_sites(rng, shape, density)
            for metric in R.METRICS:
                for limit in (0, 4):
                    assert np.array_equal(R.ref_separable(img, metric, 0, limit), R.ref_brute(img, metric, 0, limit))


@pytest.mark.parametrize("shape,density", [((1, 200, 300, 1), 0.001), ((2, 70, 129, 3), 0.02), ((1, 33, 257, 4), 0.2), ((1, 150, 40, 2), 0.0005)])
def test_cpu_device_equals_the_separable_restatement(pkg, L, shape, density):
    rng = np.random.default_rng(shape[1] + shape[2])
    img = random_sites(rng, shape, density)
    for metric in R.METRICS:
        for limit in (0, 20):
            assert np.array_equal(cpu_table(pkg, L, img, metric, 0, limit, n_threads=4), R.ref_separable(img, metric, 0, limit)), (metric, limit)


def test_scipy_gives_the_same_distances(pkg, L):
    """The independent yardstick: scipy's exact Euclidean transform, squared and rounded, and its two chamfer transforms,
    which are exact for the chessboard and the taxicab metric."""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(11)
    for h, w, density in ((37, 53, 0.01), (64, 48, 0.1), (5, 90, 0.03)):
        img = random_sites(rng, (1, h, w, 1), density)
        img[0, h // 2, w // 3, 0] = 0                                           # at least one site
        far = img[0, :, :, 0] != 0                                              # scipy measures to the nearest ZERO of its input
        assert np.array_equal(cpu_table(pkg, L, img, R.L2)[0, :, :, 0], np.rint(ndi.distance_transform_edt(far) ** 2).astype(np.uint32))
        assert np.array_equal(cpu_table(pkg, L, img, R.LINF)[0, :, :, 0], ndi.distance_transform_cdt(far, "chessboard").astype(np.uint32))
        assert np.array_equal(cpu_table(pkg, L, img, R.L1)[0, :, :, 0], ndi.distance_transform_cdt(far, "taxicab").astype(np.uint32))


# ---------------------------------------------------------------- named cases
def test_named_cases(pkg, L):
    for metric in R.METRICS:
        # 1 x 1 with and without a site
        assert cpu_table(pkg, L, np.zeros((1, 1, 1, 1), np.uint8), metric).tolist() == [[[[0]]]]
        assert cpu_table(pkg, L, np.ones((1, 1, 1, 1), np.uint8), metric).tolist() == [[[[R.NONE]]]]
        # one row, one column, a single site at each corner
        for shape in ((1, 1, 23, 1), (1, 23, 1, 1), (1, 7, 11, 2)):
            n, h, w, c = shape
            for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
                img = one_site(shape, [(0, y, x, 0)])
                got = cpu_table(pkg, L, img, metric)
                assert np.array_equal(got, R.ref_brute(img, metric))
                assert got[0, h - 1 - y, w - 1 - x, 0] == R.combine(metric, w - 1, h - 1) and got[0, y, x, 0] == 0
                if c > 1:
                    assert (got[..., 1] == R.NONE).all()                           # the channel next to it has no site
        # channels with different sites next to a channel without one
        for c in (2, 3, 4):
            img = one_site((1, 9, 12, c), [(0, 2, 3, 0)] + ([(0, 8, 11, c - 1)] if c > 2 else []))
            got = cpu_table(pkg, L, img, metric)
            assert np.array_equal(got, R.ref_brute(img, metric)) and (got[..., 1] == R.NONE).all() and got[0, 2, 3, 0] == 0
        # image 0 full of sites, image 1 empty: nothing leaks across images
        img = np.stack([np.zeros((6, 10, 3), np.uint8), np.full((6, 10, 3), 9, np.uint8)])
        got = cpu_table(pkg, L, img, metric)
        assert not got[0].any() and (got[1] == R.NONE).all()
        assert not cpu_table(pkg, L, img, metric, nonzero=1)[1].any() and (cpu_table(pkg, L, img, metric, nonzero=1)[0] == R.NONE).all()
    # the 3-4-5 triangle
    img = one_site((1, 12, 12, 1), [(0, 2, 3, 0)])
    assert cpu_table(pkg, L, img, R.L2, limit=5)[0, 6, 6, 0] == 25 and cpu_table(pkg, L, img, R.L2, limit=4)[0, 6, 6, 0] == R.NONE
    assert cpu_table(pkg, L, img, R.L1, limit=7)[0, 6, 6, 0] == 7 and cpu_table(pkg, L, img, R.L1, limit=6)[0, 6, 6, 0] == R.NONE
    assert cpu_table(pkg, L, img, R.LINF, limit=4)[0, 6, 6, 0] == 4 and cpu_table(pkg, L, img, R.LINF, limit=3)[0, 6, 6, 0] == R.NONE
    # the own column offers g = 5, a neighbour 3 columns away g = 0: the row pass must win
    img = one_site((1, 8, 9, 1), [(0, 0, 2, 0), (0, 5, 5, 0)])
    assert [int(cpu_table(pkg, L, img, m)[0, 5, 2, 0]) for m in R.METRICS] == [9, 3, 3]
    # ties: two sites at the same distance, left and right, above and below
    img = one_site((1, 9, 9, 1), [(0, 4, 0, 0), (0, 4, 8, 0), (0, 0, 4, 0), (0, 8, 4, 0)])
    assert [int(cpu_table(pkg, L, img, m)[0, 4, 4, 0]) for m in R.METRICS] == [16, 4, 4]
    for m in R.METRICS:
        assert np.array_equal(cpu_table(pkg, L, img, m), R.ref_brute(img, m))


@pytest.mark.parametrize("shape", [(1, 1, 32768, 1), (1, 32768, 1, 1), (1, 32768, 2, 1)])
def test_extremes(pkg, L, shape):
    """The longest row and the longest column with the only site at one end, and two columns with the site at (0, 0):
    32767^2 and 32767^2 + 1 pass through 32 bits unharmed; L1 and LINF on the same."""
    n, h, w, c = shape
    img = one_site(shape, [(0, 0, 0, 0)])
    ys, xs = np.arange(h, dtype=np.int64).reshape(h, 1), np.arange(w, dtype=np.int64).reshape(1, w)
    for metric in R.METRICS:
        got = cpu_table(pkg, L, img, metric, n_threads=4)
        assert np.array_equal(got[0, :, :, 0], R.combine(metric, xs + 0 * ys, ys + 0 * xs).astype(np.uint32)), metric
    assert int(cpu_table(pkg, L, img, R.L2)[0, h - 1, w - 1, 0]) == (h - 1) ** 2 + (w - 1) ** 2 in (32767 ** 2, 32767 ** 2 + 1)
    far = one_site(shape, [(0, h - 1, w - 1, 0)])
    assert int(cpu_table(pkg, L, far, R.L2, limit=32767)[0, 0, 0, 0]) == (32767 ** 2 if min(h, w) == 1 else R.NONE)
    assert int(cpu_table(pkg, L, far, R.L2, limit=32766)[0, 0, 0, 0]) == R.NONE


# ---------------------------------------------------------------- properties
def test_linf_discs_are_the_rectangular_morphology(pkg, L):
    """On masks, dilation by the chessboard ball of radius r is the window maximum over (2 r + 1)^2 and erosion the window
    minimum: a clamp-to-edge window only repeats in-image pixels that it already holds."""
    rng = np.random.default_rng(21)
    cpu = pkg.DEVICE_CPU
    mask = np.where(rng.random((2, 45, 61, 3)) < 0.03, 255, 0).astype(np.uint8)
    holes = np.where(rng.random((2, 45, 61, 3)) < 0.03, 0, 255).astype(np.uint8)
    for r in (1, 3, 16):
        assert np.array_equal(pkg.disc_dilate(mask, r, "linf", device=cpu), pkg.dilate(mask, 2 * r + 1, device=cpu)), r
        assert np.array_equal(pkg.disc_erode(holes, r, "linf", device=cpu), pkg.erode(holes, 2 * r + 1, device=cpu)), r
    grey = mask[0, :, :, 0].copy()
    assert np.array_equal(pkg.disc_dilate(grey, 2, "linf", device=cpu), pkg.dilate(grey, 5, device=cpu))


def test_within_byte_and_in_place(pkg, L):
    rng = np.random.default_rng(22)
    img = random_sites(rng, (2, 50, 70, 3), 0.004)
    for metric in R.METRICS:
        full = cpu_table(pkg, L, img, metric)
        for r in (1, 7, 30):
            within = cpu_bytes(pkg, L, img, pkg.Dist(metric, 0, r, R.WITHIN, 0))
            assert np.array_equal(within == 255, full <= R.combine(metric, r, 0)) and np.isin(within, (0, 255)).all()
            assert np.array_equal(cpu_bytes(pkg, L, img, pkg.Dist(metric, 0, r, R.WITHIN, 1)), 255 - within)
        # a distance above 255 rounds to at least 255: the limit 255 changes no byte
        wide = one_site((1, 3, 700, 1), [(0, 1, 10, 0), (0, 2, 690, 0)])
        assert np.array_equal(cpu_bytes(pkg, L, wide, pkg.Dist(metric, 0, 255, R.BYTE, 0)), cpu_bytes(pkg, L, wide, pkg.Dist(metric, 0, 0, R.BYTE, 0)))
        assert (cpu_bytes(pkg, L, wide, pkg.Dist(metric, 0, 0, R.BYTE, 0)) == 255).any()
        # d_out == d_in
        for k in (pkg.Dist(metric, 0, 0, R.BYTE, 0), pkg.Dist(metric, 1, 9, R.WITHIN, 1)):
            want = cpu_bytes(pkg, L, img, k)
            mine = img.copy()
            n, h, w, c = mine.shape
            pkg.check(L.mi_blur_cpu_run_dist_u8(mine.ctypes.data, mine.ctypes.data, w, h, c, n, C.byref(k), 2), "mi_blur_cpu_run_dist_u8")
            assert np.array_equal(mine, want)


# ---------------------------------------------------------------- statuses
def test_invalid_arguments_leave_the_output_untouched(pkg, L):
    w, h, c, n = 16, 6, 3, 2
    img = np.zeros((n, h, w, c), np.uint8)
    big = np.zeros(3 * img.size, np.uint8)
    out = np.full(img.size, 0xA5, np.uint8)
    tab = np.full(img.size + 4, ONES, np.uint32)
    work = np.zeros(1 << 16, np.uint8)
    assert tab.ctypes.data % 16 == 0 and work.ctypes.data % 16 == 0
    i_, o_, t_, w_, b_ = img.ctypes.data, out.ctypes.data, tab.ctypes.data, work.ctypes.data, big.ctypes.data
    INV, OK = pkg.ERR_INVALID, pkg.OK
    shapes = [(0, h, c, n), (w, 0, c, n), (w, h, 0, n), (w, h, 5, n), (w, h, c, -1), (32769, 1, 1, 1), (32768, 32768, 3, 1)]
    good_t, good_b = pkg.Dist(R.L2, 0, 0, 0, 0), pkg.Dist(R.L1, 1, 4, R.WITHIN, 1)
    table_forms = [lambda k, i=i_, o=t_, ww=w, hh=h, cc=c, nn=n: L.mi_blur_cpu_run_dist(i, o, ww, hh, cc, nn, k, 1),
                   lambda k, i=i_, o=t_, ww=w, hh=h, cc=c, nn=n: L.mi_blur_enqueue_dist(i, o, ww, hh, cc, nn, k, w_, None),
                   lambda k, i=i_, o=t_, ww=w, hh=h, cc=c, nn=n: L.mi_blur_run_dist(pkg.DEVICE_CPU, i, o, ww, hh, cc, nn, k),
                   lambda k, i=i_, o=t_, ww=w, hh=h, cc=c, nn=n: L.mi_blur_run_dist(0, i, o, ww, hh, cc, nn, k)]
    byte_forms = [lambda k, i=i_, o=o_, ww=w, hh=h, cc=c, nn=n: L.mi_blur_cpu_run_dist_u8(i, o, ww, hh, cc, nn, k, 1),
                  lambda k, i=i_, o=o_, ww=w, hh=h, cc=c, nn=n: L.mi_blur_enqueue_dist_u8(i, o, ww, hh, cc, nn, k, w_, None),
                  lambda k, i=i_, o=o_, ww=w, hh=h, cc=c, nn=n: L.mi_blur_run_dist_u8(pkg.DEVICE_CPU, i, o, ww, hh, cc, nn, k),
                  lambda k, i=i_, o=o_, ww=w, hh=h, cc=c, nn=n: L.mi_blur_run_dist_u8(0, i, o, ww, hh, cc, nn, k)]
    for forms, good, bytes_form in ((table_forms, good_t, False), (byte_forms, good_b, True)):
        for f in forms:
            for k in bad_structs(pkg, bytes_form):
                assert f(C.byref(k)) == INV, (bytes_form, k.metric, k.sites_nonzero, k.limit, k.byte_op, k.invert)
            assert f(None) == INV and f(C.byref(good), i=None) == INV and f(C.byref(good), o=None) == INV
            for ww, hh, cc, nn in shapes:
                assert f(C.byref(good), ww=ww, hh=hh, cc=cc, nn=nn) == INV, (ww, hh, cc, nn)
            assert f(C.byref(good), nn=0) == OK
    # a misaligned table: 2 bytes off anywhere, 4 or 8 bytes off on the device only
    for f in table_forms:
        assert f(C.byref(good_t), o=t_ + 2) == INV
    assert table_forms[1](C.byref(good_t), o=t_ + 4) == INV and table_forms[1](C.byref(good_t), o=t_ + 8) == INV
    # the work buffer
    assert L.mi_blur_enqueue_dist(i_, t_, w, h, c, n, C.byref(good_t), None, None) == INV
    assert L.mi_blur_enqueue_dist(i_, t_, w, h, c, n, C.byref(good_t), w_ + 8, None) == INV
    assert L.mi_blur_enqueue_dist_u8(i_, o_, w, h, c, n, C.byref(good_b), None, None) == INV
    assert L.mi_blur_enqueue_dist_u8(i_, o_, w, h, c, n, C.byref(good_b), w_ + 4, None) == INV
    # an output that overlaps the input without being it
    for f in byte_forms:
        for off in (1, img.size - 1, -1):
            assert f(C.byref(good_b), i=b_ + img.size, o=b_ + img.size + off) == INV, off
    assert (out == 0xA5).all() and (tab == ONES).all() and not big.any()
    off = np.full(img.size + 4, ONES, np.uint32)
    assert L.mi_blur_cpu_run_dist(i_, off.ctypes.data + 4, w, h, c, n, C.byref(good_t), 1) == OK and off[0] == ONES and not off[1:img.size + 1].any()
    if L.mi_blur_device_count() <= 0:                  # every argument good: the device is asked for last
        assert L.mi_blur_enqueue_dist(i_, t_, w, h, c, n, C.byref(good_t), w_, None) == pkg.ERR_NO_DEVICE
        assert L.mi_blur_enqueue_dist_u8(i_, o_, w, h, c, n, C.byref(good_b), w_, None) == pkg.ERR_NO_DEVICE
        assert L.mi_blur_enqueue_dist_u8(i_, i_, w, h, c, n, C.byref(good_b), w_, None) == pkg.ERR_NO_DEVICE
        assert L.mi_blur_run_dist(0, i_, t_, w, h, c, n, C.byref(good_t)) == pkg.ERR_NO_DEVICE
        assert L.mi_blur_run_dist_u8(0, i_, o_, w, h, c, n, C.byref(good_b)) == pkg.ERR_NO_DEVICE
        assert (out == 0xA5).all() and (tab == ONES).all()


def test_work_bytes(pkg, L):
    k = pkg.Dist(R.L2, 0, 0, 0, 0)
    for shape in ((1, 1, 1, 1), (2, 16, 16, 3), (3, 17, 40, 4), (1, 4097, 4112, 1), (35, 256, 256, 3), (1, 33, 5, 1)):
        n, h, w, c = shape
        assert L.mi_blur_dist_work_bytes(w, h, c, n, C.byref(k)) == R.work_bytes(shape)
    assert L.mi_blur_dist_work_bytes(16, 16, 3, 2, C.byref(pkg.Dist(R.L1, 1, 9, R.WITHIN, 1))) == R.work_bytes((2, 16, 16, 3))
    try:
        assert L.mi_blur_set_option(b"dist_band", 4) == pkg.OK
        assert L.mi_blur_dist_work_bytes(5, 33, 1, 1, C.byref(k)) == R.work_bytes((1, 33, 5, 1), 4)
    finally:
        assert L.mi_blur_set_option(b"dist_band", R.BAND) == pkg.OK
    assert L.mi_blur_dist_work_bytes(16, 16, 3, 0, C.byref(k)) == 0 and L.mi_blur_dist_work_bytes(16, 16, 5, 1, C.byref(k)) == 0
    assert L.mi_blur_dist_work_bytes(16, 16, 3, -1, C.byref(k)) == 0 and L.mi_blur_dist_work_bytes(0, 16, 3, 1, C.byref(k)) == 0
    assert L.mi_blur_dist_work_bytes(16, 16, 3, 1, None) == 0 and L.mi_blur_dist_work_bytes(16, 16, 3, 1, C.byref(pkg.Dist(3, 0, 0, 0, 0))) == 0


# ---------------------------------------------------------------- the numpy functions on the CPU device
def test_numpy_functions(pkg, L):
    rng = np.random.default_rng(23)
    cpu = pkg.DEVICE_CPU
    stack = random_sites(rng, (3, 30, 44, 3), 0.01)
    grey = stack[0, :, :, 0].copy()
    for name, metric in (("l2", R.L2), ("l1", R.L1), ("linf", R.LINF)):
        T = pkg.distance_transform(stack, name, device=cpu, batch=2)
        assert T.dtype == np.uint32 and np.array_equal(T, R.ref_brute(stack, metric))
        assert np.array_equal(pkg.distance_transform(stack, name, "nonzero", 6, device=cpu), R.ref_brute(stack, metric, 1, 6))
        assert np.array_equal(pkg.distance_transform(stack[1], name, device=cpu), T[1])
        assert np.array_equal(pkg.distance_transform(grey, name.upper(), device=cpu), T[0, :, :, 0])
        B = pkg.distance_transform_u8(stack, name, device=cpu)
        assert B.dtype == np.uint8 and np.array_equal(B, R.ref_bytes(T, metric))
        mask = (stack == 0).astype(np.uint8) * 200                                  # any non-zero value is "set"
        assert np.array_equal(pkg.disc_dilate(mask, 4, name, device=cpu, batch=1), np.where(T <= R.combine(metric, 4, 0), 255, 0))
        assert np.array_equal(pkg.disc_erode(stack, 4, name, device=cpu), np.where(T <= R.combine(metric, 4, 0), 0, 255))
    k = pkg.Dist(R.L2, 0, 0, R.BYTE, 0)
    assert pkg.dist_value(k, 2) == 1 and pkg.dist_value(k, 3) == 2 and pkg.dist_value(k, R.NONE) == 255 and pkg.DIST_NONE == R.NONE
    bad = [lambda: pkg.distance_transform(stack, "l3", device=cpu), lambda: pkg.distance_transform(stack, 0, device=cpu),
           lambda: pkg.distance_transform(stack, sites="some", device=cpu), lambda: pkg.distance_transform(stack, limit=32768, device=cpu),
           lambda: pkg.distance_transform(stack, limit=-1, device=cpu), lambda: pkg.distance_transform_u8(stack, limit=2.0, device=cpu),
           lambda: pkg.disc_dilate(stack, 0, device=cpu), lambda: pkg.disc_erode(stack, 32768, device=cpu),
           lambda: pkg.disc_dilate(np.zeros((2, 4, 4, 5), np.uint8), 3, device=cpu), lambda: pkg.distance_transform(stack.astype(np.float32), device=cpu)]
    for f in bad:
        with pytest.raises(ValueError):
            f()


def test_constants(pkg):
    """dist_ref.py's copies of the kernels' units and of the enums."""
    text = open(os.path.join(pkg.CSRC, "filter.h")).read()
    assert f"constexpr int DIST_BAND = {R.BAND};" in text and f"constexpr int DIST_MAX_ROW = {R.MAX_ROW};" in text
    assert f"constexpr int DIST_CHUNK_LOG2 = {R.CHUNK.bit_length() - 1};" in text
    assert f"constexpr int DIST_TILE_ELEMS = {R.TILE_ELEMS};" in text and f"constexpr int DIST_MAX_ROWS = {R.MAX_ROWS};" in text
    launch = open(os.path.join(pkg.CSRC, "blur_launch.h")).read()
    assert f'{{"dist_band", &Tunables::dist_band, KnobKind::RANGE, 1, 256, {R.BAND}, nullptr}}' in launch
    assert f'{{"dist_chunk_log2", &Tunables::dist_chunk_log2, KnobKind::RANGE, 3, 5, {R.CHUNK.bit_length() - 1}, nullptr}}' in launch
    header = open(pkg.HEADER).read()
    assert "MI_BLUR_DIST_L2 = 0, MI_BLUR_DIST_L1 = 1, MI_BLUR_DIST_LINF = 2" in header and "MI_BLUR_DIST_BYTE = 0, MI_BLUR_DIST_WITHIN = 1" in header
    assert f"#define MI_BLUR_DIST_MAX_LIMIT {R.MAX_LIMIT}" in header and "#define MI_BLUR_DIST_NONE 0xFFFFFFFFu" in header
    assert (pkg.DIST_L2, pkg.DIST_L1, pkg.DIST_LINF, pkg.DIST_BYTE, pkg.DIST_WITHIN, pkg.DIST_MAX_LIMIT) == (R.L2, R.L1, R.LINF, R.BYTE, R.WITHIN, R.MAX_LIMIT)
    assert {pkg.DIST_METRICS[v] for v in R.NAMES.values()} == set(R.METRICS)
    for name in (R.TILED, R.GENERIC):
        assert f'"{name}"' in header


@needs_gxx
def test_dist_clean_under_asan_ubsan(pkg, tmp_path):
    run_sanitized(pkg, tmp_path, ("san_dist.cpp", "cpu_device.cpp"), ["arithmetic clean", "named cases clean", "extremes clean", "random cases clean"])
