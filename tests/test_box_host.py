"""The integral images and the box filters without a GPU (mi_blur_box_value, mi_blur_cpu_run_integral, mi_blur_cpu_run_box,
the blocking exports on the CPU device, integral() and its kin): the definition at every rounding boundary of every window
area, the five-term form against box_ref.py's padded sliding sums, the properties the header names, the modulus, the
statuses, the constants box_ref.py copies and the sanitizer program."""
import ctypes as C
import os

import numpy as np
import pytest

import box_ref as R
from hist_ref import ref_hist
from resample_harness import needs_gxx, run_sanitized

ONES = 0xFFFFFFFF
# every A that an (rx, ry) pair can give, with one pair that gives it
AREAS = {}
for _rx in range(R.MAX_RADIUS + 1):
    for _ry in range(_rx + 1):
        AREAS.setdefault((2 * _rx + 1) * (2 * _ry + 1), (_rx, _ry))
RADII = [(0, 0), (1, 1), (1, 7), (3, 2), (16, 16), (127, 0), (0, 127), (127, 127)]
OPS = (R.MEAN, R.STDDEV, R.THRESHOLD)


def spec(pkg, op, rx, ry):
    """A struct of op that uses what the mode has: an offset and, for odd rx, invert."""
    return pkg.Box(op, rx, ry, -3, rx & 1) if op == R.THRESHOLD else pkg.Box(op, rx, ry, 0, 0)


def cpu_box(pkg, L, img, k, n_threads=3, guard=64):
    """mi_blur_cpu_run_box into a buffer of 0xA5 with `guard` bytes either side of the output."""
    a = np.ascontiguousarray(img)
    n, h, w, c = a.shape
    buf = np.full(a.size + 2 * guard, 0xA5, np.uint8)
    pkg.check(L.mi_blur_cpu_run_box(a.ctypes.data, buf.ctypes.data + guard, w, h, c, n, C.byref(k), n_threads), "mi_blur_cpu_run_box")
    assert (buf[:guard] == 0xA5).all() and (buf[guard + a.size:] == 0xA5).all(), "wrote outside the output"
    return buf[guard:guard + a.size].reshape(a.shape)


def cpu_integral(pkg, L, img, want_s=True, want_q=True, n_threads=3, guard=16):
    """mi_blur_cpu_run_integral into tables of 0xFFFFFFFF words with `guard` words either side: (S, Q), None where not asked."""
    a = np.ascontiguousarray(img)
    n, h, w, c = a.shape
    bufs = [np.full(a.size + 2 * guard, ONES, np.uint32) if on else None for on in (want_s, want_q)]
    ptr = [None if b is None else b.ctypes.data + 4 * guard for b in bufs]
    pkg.check(L.mi_blur_cpu_run_integral(a.ctypes.data, ptr[0], ptr[1], w, h, c, n, n_threads), "mi_blur_cpu_run_integral")
    for b in bufs:
        assert b is None or ((b[:guard] == ONES).all() and (b[guard + a.size:] == ONES).all()), "wrote outside the table"
    return tuple(None if b is None else b[guard:guard + a.size].reshape(a.shape) for b in bufs)


def ref_spec(img, k):
    return R.ref_box(img, k.op, k.rx, k.ry, k.offset, k.invert)


# ---------------------------------------------------------------- the definition, one byte at a time
def test_value_mean_at_every_rounding_boundary(pkg, L):
    """For every A and every v in 1..255: the smallest Sum that gives v, (A (2 v - 1) + 1) / 2 (A is odd), and the largest
    that gives v - 1, one below it; and Sum = 0 and 255 A."""
    assert len(AREAS) > 4000 and min(AREAS) == 1 and max(AREAS) == 65025
    call = L.mi_blur_box_value
    v = np.arange(1, 256, dtype=np.int64)
    for A, (rx, ry) in AREAS.items():
        k = C.byref(pkg.Box(R.MEAN, rx, ry, 0, 0))
        first = (A * (2 * v - 1) + 1) // 2
        assert np.array_equal(R.ref_value(R.MEAN, A, first), v) and np.array_equal(R.ref_value(R.MEAN, A, first - 1), v - 1)
        got = [call(k, A, s, 0, 0) for s in first.tolist()]
        below = [call(k, A, s - 1, 0, 0) for s in first.tolist()]
        assert got == v.tolist() and below == (v - 1).tolist(), A
        assert call(k, A, 0, 0, 0) == 0 and call(k, A, 255 * A, 0, 0) == 255 and call(k, A, 255 * A + 1, 0, 0) == -1


def test_value_stddev_at_every_threshold(pkg, L):
    """For every A and every s in 1..128 the threshold is D >= T = ((2 s - 1)^2 A^2 + 3) / 4 (the square is 1 modulo 4).
    D = A SumSq - Sum^2 takes only the values -Sum^2 modulo A, so per (A, s) the test takes, over Sum in 0..7, the D
    nearest at or above T and the D nearest below it, and wants the count of thresholds at or below D: the restated rule."""
    call = L.mi_blur_box_value
    s = np.arange(1, 129, dtype=np.int64)[:, None]
    t = np.arange(8, dtype=np.int64)[None, :]
    exact = 0
    for A, (rx, ry) in AREAS.items():
        k = C.byref(pkg.Box(R.STDDEV, rx, ry, 0, 0))
        T = ((2 * s - 1) ** 2 * A * A + 3) // 4
        q_hi = -(-(T + t * t) // A)
        d_hi = A * q_hi - t * t
        d_hi[(q_hi > 65025 * A) | (t > 255 * A)] = 1 << 62
        q_lo = (T - 1 + t * t) // A
        d_lo = A * q_lo - t * t
        d_lo[(d_lo < 0) | (t > 255 * A)] = -1 << 62
        pick_hi, pick_lo = d_hi.argmin(axis=1), d_lo.argmax(axis=1)
        rows = np.arange(128)
        D_hi, D_lo = d_hi[rows, pick_hi], d_lo[rows, pick_lo]
        assert (D_hi >= T[:, 0]).all() and (D_hi < T[:, 0] + A).all() and (D_lo < T[:, 0]).all() and (D_lo >= np.maximum(T[:, 0] - A, 0)).all()
        exact += int((D_hi == T[:, 0]).sum()) + int((D_lo == T[:, 0] - 1).sum())
        want_hi, want_lo = np.searchsorted(T[:, 0], D_hi, side="right"), np.searchsorted(T[:, 0], D_lo, side="right")
        assert (want_hi >= s[:, 0]).all() and (want_lo < s[:, 0]).all()
        got_hi = [call(k, A, int(pick_hi[i]), int(q_hi[i, pick_hi[i]]), 0) for i in range(128)]
        got_lo = [call(k, A, int(pick_lo[i]), int(q_lo[i, pick_lo[i]]), 0) for i in range(128)]
        assert got_hi == want_hi.tolist() and got_lo == want_lo.tolist(), A
    assert exact >= 256                     # A = 1 alone meets every threshold, and the D below it, exactly
    # the restated rule itself, against the root in floating point far from the thresholds
    A = 25
    D = np.array([0, 1, 156, 157, 25 * 25 * 100, 25 * 25 * 16256], np.int64)
    assert R.ref_stddev(A, np.zeros(6, np.int64), D // A).tolist() == [0, 0, 0, 0, 10, 127]
    k = pkg.Box(R.STDDEV, 2, 2, 0, 0)
    assert L.mi_blur_box_value(C.byref(k), 25, 10, 3, 0) == -1             # Sum^2 > A SumSq: no window has such sums
    assert L.mi_blur_box_value(C.byref(k), 25, 0, 65025 * 25 + 1, 0) == -1


def test_value_threshold_around_equality(pkg, L):
    """A (a + offset) - Sum in {-1, 0, 1}, both polarities, for every A."""
    call = L.mi_blur_box_value
    for A, (rx, ry) in AREAS.items():
        for a, offset in ((0, 0), (255, 0), (128, -37), (10, 200), (200, -150), (1, -1), (0, 255), (255, -255)):
            for invert in (0, 1):
                k = C.byref(pkg.Box(R.THRESHOLD, rx, ry, offset, invert))
                for d in (-1, 0, 1):
                    Sum = A * (a + offset) - d
                    if not 0 <= Sum <= 255 * A:
                        continue
                    want = 255 if (d > 0) != bool(invert) else 0
                    assert int(R.ref_value(R.THRESHOLD, A, Sum, 0, a, offset, invert)) == want
                    assert call(k, A, Sum, 0, a) == want, (A, a, offset, invert, d)
    k = pkg.Box(R.THRESHOLD, 1, 1, 0, 0)
    assert L.mi_blur_box_value(C.byref(k), 9, 0, 0, 256) == -1 and L.mi_blur_box_value(C.byref(k), 9, 0, 0, -1) == -1
    assert L.mi_blur_box_value(C.byref(k), 25, 0, 0, 0) == -1 and L.mi_blur_box_value(None, 9, 0, 0, 0) == -1
    assert L.mi_blur_box_value(C.byref(pkg.Box(R.MEAN, 1, 1, 1, 0)), 9, 0, 0, 0) == -1


# ---------------------------------------------------------------- the five-term form against padded sliding sums
@pytest.mark.parametrize("w,h", [(1, 1), (1, 9), (9, 1), (7, 9), (16, 4), (23, 17), (40, 33)])
def test_five_term_form_equals_the_sliding_sums(pkg, L, w, h):
    """Images smaller than, equal to and larger than the window, every pixel, all three modes (r = 127 on 16 x 4 included)."""
    rng = np.random.default_rng(1000 * w + h)
    for c in ((1, 2, 3, 4) if (w, h) in ((7, 9), (16, 4)) else (3,)):
        img = rng.integers(0, 256, size=(2, h, w, c), dtype=np.uint8)
        img[1, h // 2:] = (img[1, h // 2:] // 8 + 100).astype(np.uint8)               # a flat half: small deviations too
        for rx, ry in RADII + [((w - 1) // 2, (h - 1) // 2)]:
            for op in OPS:
                k = spec(pkg, op, rx, ry)
                assert np.array_equal(cpu_box(pkg, L, img, k), ref_spec(img, k)), (c, rx, ry, op)


def test_integral_equals_the_cumulative_sums(pkg, L):
    rng = np.random.default_rng(7)
    for n, h, w, c in ((2, 1, 1, 1), (2, 5, 7, 3), (3, 37, 16, 4), (1, 70, 33, 2), (2, 129, 48, 1)):
        img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
        for threads in (1, 5):
            S, Q = cpu_integral(pkg, L, img, n_threads=threads)
            assert np.array_equal(S, R.ref_integral(img)) and np.array_equal(Q, R.ref_integral(img, True)), (n, h, w, c)
        assert np.array_equal(cpu_integral(pkg, L, img, True, False)[0], S) and np.array_equal(cpu_integral(pkg, L, img, False, True)[1], Q)


# ---------------------------------------------------------------- properties
def test_radius_zero_and_constant_images(pkg, L):
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, size=(2, 9, 20, 3), dtype=np.uint8)
    assert np.array_equal(cpu_box(pkg, L, img, pkg.Box(R.MEAN, 0, 0, 0, 0)), img)
    assert not cpu_box(pkg, L, img, pkg.Box(R.STDDEV, 0, 0, 0, 0)).any()
    assert not cpu_box(pkg, L, img, pkg.Box(R.THRESHOLD, 0, 0, 0, 0)).any()
    assert (cpu_box(pkg, L, img, pkg.Box(R.THRESHOLD, 0, 0, 0, 1)) == 255).all()
    for level in (0, 1, 77, 254, 255):
        flat = np.full((1, 12, 18, 2), level, np.uint8)
        for rx, ry in ((1, 1), (5, 2), (127, 127)):
            assert (cpu_box(pkg, L, flat, pkg.Box(R.MEAN, rx, ry, 0, 0)) == level).all()
            assert not cpu_box(pkg, L, flat, pkg.Box(R.STDDEV, rx, ry, 0, 0)).any()


def test_box_blur_of_three_is_the_area_resize_to_a_third(pkg, L):
    """Both are the mean of a 3 x 3 block rounded half up, on a size divisible by 3."""
    rng = np.random.default_rng(12)
    cpu = pkg.DEVICE_CPU
    img = rng.integers(0, 256, size=(2, 27, 36, 3), dtype=np.uint8)
    assert np.array_equal(pkg.box_blur(img, 3, device=cpu)[:, 1::3, 1::3], pkg.area_resize(img, (12, 9), device=cpu))


def test_last_entry_is_the_histograms_moment(pkg, L):
    rng = np.random.default_rng(13)
    cpu = pkg.DEVICE_CPU
    img = rng.integers(0, 256, size=(2, 300, 420, 3), dtype=np.uint8)
    hist = pkg.histogram(img, device=cpu).astype(np.uint64)
    assert np.array_equal(hist, ref_hist(img))
    v = np.arange(256, dtype=np.uint64)
    S, Q = pkg.integral(img, device=cpu), pkg.integral(img, square=True, device=cpu)
    assert np.array_equal(S[:, -1, -1, :], ((hist * v).sum(axis=2) % R.M32).astype(np.uint32))
    assert np.array_equal(Q[:, -1, -1, :], ((hist * v * v).sum(axis=2) % R.M32).astype(np.uint32))


def test_stddev_of_a_step_by_hand(pkg, L):
    """Columns 0..15 are 0, 16..31 are 255; a 5 x 5 window with k columns of 255 has mean 51 k and deviation
    51 sqrt(k (5 - k)): 102 for k = 1 and 4, 124.9 -> 125 for k = 2 and 3, 0 away from the step."""
    img = np.zeros((1, 8, 32, 1), np.uint8)
    img[:, :, 16:] = 255
    got = cpu_box(pkg, L, img, pkg.Box(R.STDDEV, 2, 2, 0, 0))
    row = [0] * 14 + [102, 125, 125, 102] + [0] * 14
    assert (got[0, :, :, 0] == np.array(row, np.uint8)).all()
    wide = cpu_box(pkg, L, img, pkg.Box(R.STDDEV, 16, 0, 0, 0))                        # 33 columns: at x = 15 sixteen of them are 255
    assert wide[0, 0, 15, 0] == round(255 * (16 * 17) ** 0.5 / 33) == 127 and wide[0, 0, 0, 0] == round(255 * 32 ** 0.5 / 33)
    mean = cpu_box(pkg, L, img, pkg.Box(R.MEAN, 2, 2, 0, 0))
    assert mean[0, 3, 12:20, 0].tolist() == [0, 0, 51, 102, 153, 204, 255, 255]


# ---------------------------------------------------------------- the modulus
def test_tables_wrap_and_windows_stay_exact(pkg, L):
    h, w = 4097, 4112
    assert h * w * 255 > R.M32
    img = np.full((1, h, w, 1), 255, np.uint8)
    S = np.empty(img.shape, np.uint32)
    pkg.check(L.mi_blur_cpu_run_integral(img.ctypes.data, S.ctypes.data, None, w, h, 1, 1, 0), "mi_blur_cpu_run_integral")
    assert np.array_equal(S, R.ref_integral(img))
    assert (np.diff(S[0, -1, :, 0].astype(np.int64)) < 0).any(), "the last row never wrapped"
    assert int(S[0, -1, -1, 0]) == h * w * 255 - R.M32
    out = pkg.box_blur(img, (255, 31), device=pkg.DEVICE_CPU)
    assert out.shape == img.shape and (out == 255).all()


# ---------------------------------------------------------------- statuses
def test_invalid_arguments_leave_the_output_untouched(pkg, L):
    w, h, c, n = 16, 6, 3, 2
    img = np.zeros((n, h, w, c), np.uint8)
    out = np.full(img.size, 0xA5, np.uint8)
    tab = np.full(img.size + 4, ONES, np.uint32)
    tab2 = np.full(img.size + 4, ONES, np.uint32)
    work = np.zeros(1 << 16, np.uint8)
    assert tab.ctypes.data % 16 == 0 and tab2.ctypes.data % 16 == 0 and work.ctypes.data % 16 == 0
    i_, o_, t_, q_, w_ = img.ctypes.data, out.ctypes.data, tab.ctypes.data, tab2.ctypes.data, work.ctypes.data
    INV, OK = pkg.ERR_INVALID, pkg.OK
    good = pkg.Box(R.MEAN, 1, 1, 0, 0)
    bad_structs = [pkg.Box(3, 1, 1, 0, 0), pkg.Box(-1, 1, 1, 0, 0), pkg.Box(R.MEAN, 128, 1, 0, 0), pkg.Box(R.MEAN, 1, 128, 0, 0),
                   pkg.Box(R.MEAN, -1, 1, 0, 0), pkg.Box(R.THRESHOLD, 1, 1, 256, 0), pkg.Box(R.THRESHOLD, 1, 1, -256, 0),
                   pkg.Box(R.THRESHOLD, 1, 1, 0, 2), pkg.Box(R.THRESHOLD, 1, 1, 0, -1), pkg.Box(R.MEAN, 1, 1, 1, 0), pkg.Box(R.MEAN, 1, 1, 0, 1),
                   pkg.Box(R.STDDEV, 1, 1, -1, 0), pkg.Box(R.STDDEV, 1, 1, 0, 1)]
    shapes = [(0, h, c, n), (w, 0, c, n), (w, h, 0, n), (w, h, 5, n), (w, h, c, -1), (32769, 1, 1, 1), (32768, 32768, 3, 1)]
    # the integral: null combinations, a misaligned table, the image, the batch
    for f in (lambda *a: L.mi_blur_cpu_run_integral(*a, 1), lambda *a: L.mi_blur_enqueue_integral(*a, w_, None),
              lambda *a: L.mi_blur_run_integral(pkg.DEVICE_CPU, *a), lambda *a: L.mi_blur_run_integral(0, *a)):
        assert f(None, t_, q_, w, h, c, n) == INV and f(i_, None, None, w, h, c, n) == INV
        assert f(i_, t_ + 2, None, w, h, c, n) == INV and f(i_, None, q_ + 1, w, h, c, n) == INV and f(i_, t_, q_ + 3, w, h, c, n) == INV
        for ww, hh, cc, nn in shapes:
            assert f(i_, t_, q_, ww, hh, cc, nn) == INV, (ww, hh, cc, nn)
        assert f(i_, t_, q_, w, h, c, 0) == OK
    # a table 4 or 8 bytes off is fine in host memory, not on the device
    assert L.mi_blur_enqueue_integral(i_, t_ + 4, None, w, h, c, n, w_, None) == INV and L.mi_blur_enqueue_integral(i_, t_, q_ + 8, w, h, c, n, w_, None) == INV
    assert L.mi_blur_enqueue_integral(i_, t_, q_, w, h, c, n, None, None) == INV and L.mi_blur_enqueue_integral(i_, t_, q_, w, h, c, n, w_ + 8, None) == INV
    assert (tab == ONES).all() and (tab2 == ONES).all()
    off = np.full(img.size + 4, ONES, np.uint32)
    assert L.mi_blur_cpu_run_integral(i_, off.ctypes.data + 4, None, w, h, c, n, 1) == OK and off[0] == ONES and not off[1:img.size + 1].any()
    # the box filters
    forms = [lambda k, ww=w, hh=h, cc=c, nn=n, i=i_, o=o_: L.mi_blur_cpu_run_box(i, o, ww, hh, cc, nn, k, 1),
             lambda k, ww=w, hh=h, cc=c, nn=n, i=i_, o=o_: L.mi_blur_enqueue_box(i, o, ww, hh, cc, nn, k, w_, None),
             lambda k, ww=w, hh=h, cc=c, nn=n, i=i_, o=o_: L.mi_blur_run_box(pkg.DEVICE_CPU, i, o, ww, hh, cc, nn, k),
             lambda k, ww=w, hh=h, cc=c, nn=n, i=i_, o=o_: L.mi_blur_run_box(0, i, o, ww, hh, cc, nn, k)]
    for f in forms:
        for k in bad_structs:
            assert f(C.byref(k)) == INV, (k.op, k.rx, k.ry, k.offset, k.invert)
        assert f(None) == INV and f(C.byref(good), i=None) == INV and f(C.byref(good), o=None) == INV
        for ww, hh, cc, nn in shapes:
            assert f(C.byref(good), ww, hh, cc, nn) == INV
        assert f(C.byref(good), nn=0) == OK
    assert L.mi_blur_enqueue_box(i_, o_, w, h, c, n, C.byref(good), None, None) == INV
    assert L.mi_blur_enqueue_box(i_, o_, w, h, c, n, C.byref(good), w_ + 4, None) == INV
    from_tables = lambda k, i, s, q, o=o_, nn=n: L.mi_blur_enqueue_box_from_integral(i, s, q, o, w, h, c, nn, k, None)
    std, thr = pkg.Box(R.STDDEV, 1, 1, 0, 0), pkg.Box(R.THRESHOLD, 1, 1, 5, 1)
    for k in bad_structs:
        assert from_tables(C.byref(k), None, t_, None) == INV
    assert from_tables(C.byref(good), None, None, None) == INV and from_tables(C.byref(good), None, t_, None, o=None) == INV
    assert from_tables(C.byref(good), i_, t_, None) == INV and from_tables(C.byref(good), None, t_, q_) == INV        # MEAN takes S alone
    assert from_tables(C.byref(std), None, t_, None) == INV and from_tables(C.byref(std), i_, t_, q_) == INV          # STDDEV: Q, no image
    assert from_tables(C.byref(thr), None, t_, None) == INV and from_tables(C.byref(thr), i_, t_, q_) == INV          # THRESHOLD: the image, no Q
    assert from_tables(C.byref(good), None, t_ + 4, None) == INV and from_tables(C.byref(std), None, t_, q_ + 8) == INV
    assert from_tables(C.byref(good), None, t_, None, nn=-1) == INV
    for k, i, q in ((good, None, None), (std, None, q_), (thr, i_, None)):
        assert from_tables(C.byref(k), i, t_, q, nn=0) == OK
    assert (out == 0xA5).all()
    if L.mi_blur_device_count() <= 0:                  # every argument good: the device is asked for last (host memory: not with a GPU)
        for k, i, q in ((good, None, None), (std, None, q_), (thr, i_, None)):
            assert from_tables(C.byref(k), i, t_, q) == pkg.ERR_NO_DEVICE
        assert L.mi_blur_enqueue_box(i_, o_, w, h, c, n, C.byref(good), w_, None) == pkg.ERR_NO_DEVICE
        assert L.mi_blur_enqueue_integral(i_, t_, q_, w, h, c, n, w_, None) == pkg.ERR_NO_DEVICE
        assert L.mi_blur_run_integral(0, i_, t_, None, w, h, c, n) == pkg.ERR_NO_DEVICE


def test_work_bytes(pkg, L):
    for shape in ((1, 1, 1, 1), (2, 16, 16, 3), (3, 17, 40, 4), (1, 4097, 4112, 1), (35, 256, 256, 3)):
        n, h, w, c = shape
        words = n * h * w * c
        table = (4 * words + 15) // 16 * 16
        for both in (0, 1):
            assert L.mi_blur_integral_work_bytes(w, h, c, n, both) == R.work_bytes(shape, 1 + both)
        for op in OPS:
            k = pkg.Box(op, 3, 3, 0, 0)
            tables = 2 if op == R.STDDEV else 1
            assert L.mi_blur_box_work_bytes(w, h, c, n, C.byref(k)) == tables * table + R.work_bytes(shape, tables)
    assert L.mi_blur_integral_work_bytes(16, 16, 3, 0, 1) == 0 and L.mi_blur_integral_work_bytes(16, 16, 5, 1, 1) == 0
    assert L.mi_blur_integral_work_bytes(16, 16, 3, -1, 0) == 0 and L.mi_blur_integral_work_bytes(0, 16, 3, 1, 0) == 0
    assert L.mi_blur_box_work_bytes(16, 16, 3, 1, None) == 0 and L.mi_blur_box_work_bytes(16, 16, 3, 1, C.byref(pkg.Box(R.MEAN, 128, 0, 0, 0))) == 0
    assert L.mi_blur_box_work_bytes(16, 16, 3, -1, C.byref(pkg.Box(R.MEAN, 1, 0, 0, 0))) == 0


# ---------------------------------------------------------------- the numpy functions on the CPU device
def test_numpy_functions(pkg, L):
    rng = np.random.default_rng(14)
    cpu = pkg.DEVICE_CPU
    stack = rng.integers(0, 256, size=(3, 30, 44, 3), dtype=np.uint8)
    grey = stack[0, :, :, 0].copy()
    S = pkg.integral(stack, device=cpu, batch=2)
    assert S.dtype == np.uint32 and np.array_equal(S, R.ref_integral(stack))
    assert np.array_equal(pkg.integral(stack, square=True, device=cpu), R.ref_integral(stack, True))
    P = pkg.integral(grey, pad=True, device=cpu)
    assert P.shape == (31, 45) and not P[0].any() and not P[:, 0].any() and np.array_equal(P[1:, 1:], R.ref_integral(grey[None, :, :, None])[0, :, :, 0])
    assert np.array_equal(pkg.integral(stack[1], device=cpu), S[1])
    for x0, y0, x1, y1 in ((0, 0, 43, 29), (0, 0, 0, 0), (5, 7, 20, 8), (43, 29, 43, 29), (0, 3, 10, 3)):
        want = stack[:, y0:y1 + 1, x0:x1 + 1].astype(np.int64).sum(axis=(1, 2))
        assert np.array_equal(pkg.rect_sum(S, x0, y0, x1, y1), want)
        assert pkg.rect_sum(pkg.integral(grey, device=cpu), x0, y0, x1, y1) == grey[y0:y1 + 1, x0:x1 + 1].astype(np.int64).sum()
    assert np.array_equal(pkg.box_blur(stack, 5, device=cpu, batch=2), R.ref_box(stack, R.MEAN, 2, 2))
    assert np.array_equal(pkg.box_blur(stack, (31, 3), device=cpu), R.ref_box(stack, R.MEAN, 15, 1))
    assert np.array_equal(pkg.box_blur(grey, 255, device=cpu), R.ref_box(grey[None, :, :, None], R.MEAN, 127, 127)[0, :, :, 0])
    assert np.array_equal(pkg.local_stddev(stack, (7, 9), device=cpu), R.ref_box(stack, R.STDDEV, 3, 4))
    assert np.array_equal(pkg.adaptive_threshold(stack, 11, 7, device=cpu), R.ref_box(stack, R.THRESHOLD, 5, 5, 7, 0))
    assert np.array_equal(pkg.adaptive_threshold(stack[0], (3, 201), -2, True, device=cpu), R.ref_box(stack[:1], R.THRESHOLD, 1, 100, -2, 1)[0])
    bad = [lambda: pkg.box_blur(stack, 4, device=cpu), lambda: pkg.box_blur(stack, 257, device=cpu), lambda: pkg.box_blur(stack, (3, 0), device=cpu),
           lambda: pkg.box_blur(stack, 3.0, device=cpu), lambda: pkg.adaptive_threshold(stack, 3, 256, device=cpu),
           lambda: pkg.local_stddev(np.zeros((2, 4, 4, 5), np.uint8), 3, device=cpu), lambda: pkg.rect_sum(S, 3, 0, 2, 0),
           lambda: pkg.rect_sum(S, 0, 0, 44, 0), lambda: pkg.rect_sum(S.astype(np.int64), 0, 0, 1, 1)]
    for f in bad:
        with pytest.raises(ValueError):
            f()


def test_constants(pkg):
    """box_ref.py's copies of the kernels' units and of the enum."""
    text = open(os.path.join(pkg.CSRC, "filter.h")).read()
    assert f"constexpr int INTEGRAL_BAND = {R.BAND};" in text and f"constexpr int INTEGRAL_MAX_W = {R.MAX_W};" in text
    assert f"constexpr int INTEGRAL_PIXELS = {R.PIXELS};" in text
    assert f'{{"integral_band", &Tunables::integral_band, KnobKind::RANGE, 1, 256, {R.BAND}, nullptr}}' in open(os.path.join(pkg.CSRC, "blur_launch.h")).read()
    header = open(pkg.HEADER).read()
    assert "MI_BLUR_BOX_MEAN = 0, MI_BLUR_BOX_STDDEV = 1, MI_BLUR_BOX_THRESHOLD = 2" in header and f"#define MI_BLUR_BOX_MAX_RADIUS {R.MAX_RADIUS}" in header
    assert (pkg.BOX_MEAN, pkg.BOX_STDDEV, pkg.BOX_THRESHOLD, pkg.BOX_MAX_RADIUS) == (R.MEAN, R.STDDEV, R.THRESHOLD, R.MAX_RADIUS)
    for name in (R.INTEGRAL_TILED, R.INTEGRAL_GENERIC, R.BOX_TILED, R.BOX_GENERIC):
        assert f'"{name}"' in header


@needs_gxx
def test_box_clean_under_asan_ubsan(pkg, tmp_path):
    run_sanitized(pkg, tmp_path, ("san_box.cpp", "cpu_device.cpp"), ["arithmetic clean", "geometry clean", "integral and box cases clean"])
