"""The histogram family without a GPU (mi_blur_cpu_run_hist / _tables / _tone, mi_blur_tone_tables, the blocking exports on
the CPU device, histogram() and its kin): exact counts and exact tables against hist_ref.py, the statuses, the constants
hist_ref.py copies, and the sanitizer program."""
import ctypes as C
import os

import numpy as np
import pytest

from color_ref import ref_preset
from hist_ref import (BINS, CLIP_MAX, EQUALIZE, GROUP, IMAGE_BLOCKS, RUN, STRETCH, ref_apply, ref_hist, ref_table, ref_tables, ref_tone)
from resample_harness import needs_gxx, no_scratch, run_sanitized

GUARD = 0xDEADBEEF
IDENT = np.arange(BINS, dtype=np.uint8)


def cpu_hist(pkg, L, img, n_threads):
    """mi_blur_cpu_run_hist into a buffer pre-filled with ones, a guard word behind it."""
    a = np.ascontiguousarray(img)
    n, h, w, c = a.shape
    buf = np.full(n * c * BINS + 1, 0xFFFFFFFF, np.uint32)
    buf[-1] = GUARD
    pkg.check(L.mi_blur_cpu_run_hist(a.ctypes.data, buf.ctypes.data, w, h, c, n, n_threads), "mi_blur_cpu_run_hist")
    assert buf[-1] == GUARD, "wrote outside the histogram"
    return buf[:-1].reshape(n, c, BINS)


def tables_of(pkg, L, hist, mode, clip_lo=0, clip_hi=0, joint=0, mask=0):
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    c = hist.shape[0]
    out = np.full(c * BINS + 16, 0xA5, np.uint8)
    t = pkg.Tone(mode, clip_lo, clip_hi, joint, mask)
    pkg.check(L.mi_blur_tone_tables(hist.ctypes.data, c, C.byref(t), out.ctypes.data), "mi_blur_tone_tables")
    assert (out[c * BINS:] == 0xA5).all()
    return out[:c * BINS].reshape(c, BINS)


def hist_of_levels(levels):
    """One channel: levels = {value: count}."""
    h = np.zeros((1, BINS), np.uint32)
    for v, k in levels.items():
        h[0, v] = k
    return h


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_cpu_hist_equals_bincount(pkg, L, c):
    rng = np.random.default_rng(70 + c)
    for n, h, w in ((1, 1, 1), (3, 5, 7), (2, 64, 96), (1, 300, 257)):
        img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
        want = ref_hist(img)
        assert want.sum() == img.size
        for nt in (1, 4):
            assert np.array_equal(cpu_hist(pkg, L, img, nt), want), (n, h, w, nt)


def test_tables_exact_cases(pkg, L):
    for mode in (EQUALIZE, STRETCH):
        # one level: the identity
        assert np.array_equal(tables_of(pkg, L, hist_of_levels({77: 1234}), mode)[0], IDENT)
        # two levels: 0 up to the first, 255 from the second on, both modes
        got = tables_of(pkg, L, hist_of_levels({40: 10, 200: 30}), mode)[0]
        assert np.array_equal(got, ref_table(hist_of_levels({40: 10, 200: 30})[0], mode))
        assert (got[:41] == 0).all() and (got[200:] == 255).all()
        # first level 255 / last level 0
        for lv in ({255: 9}, {0: 9}, {0: 5, 255: 1}):
            assert np.array_equal(tables_of(pkg, L, hist_of_levels(lv), mode)[0], ref_table(hist_of_levels(lv)[0], mode)), lv
        assert tables_of(pkg, L, hist_of_levels({0: 5, 255: 1}), mode)[0][255] == 255
    # all 256 levels once: EQUALIZE is the identity
    flat = np.ones((1, BINS), np.uint32)
    assert np.array_equal(tables_of(pkg, L, flat, EQUALIZE)[0], IDENT)
    assert np.array_equal(tables_of(pkg, L, flat, EQUALIZE)[0], ref_table(flat[0], EQUALIZE))
    # an all-zero histogram (no image has one): the identity
    assert np.array_equal(tables_of(pkg, L, np.zeros((1, BINS), np.uint32), EQUALIZE)[0], IDENT)
    assert np.array_equal(tables_of(pkg, L, np.zeros((1, BINS), np.uint32), STRETCH, 100, 100)[0], IDENT)


def test_tables_stretch(pkg, L):
    rng = np.random.default_rng(71)
    # clips 0: (v - min) * 255 / (max - min), rounded half up
    h = np.zeros((1, BINS), np.uint32)
    h[0, 30:181] = rng.integers(1, 50, size=151)
    got = tables_of(pkg, L, h, STRETCH)[0].astype(np.int64)
    v = np.arange(BINS, dtype=np.int64)
    want = np.clip((2 * (v - 30) * 255 + 150) // (2 * 150), 0, 255)
    assert np.array_equal(got, want) and got[30] == 0 and got[180] == 255
    # clips that land exactly on a bin boundary: N = 65536, so k = clip; c(10) = 100
    h = np.zeros((1, BINS), np.uint32)
    h[0, 10], h[0, 20], h[0, 30], h[0, 240] = 100, 65536 - 100 - 50 - 60, 50, 60
    assert int(h.sum()) == 65536
    for clip_lo, lo in ((99, 10), (100, 20), (101, 20)):                  # c(10) == k_lo + 1, == k_lo, < k_lo
        got = tables_of(pkg, L, h, STRETCH, clip_lo, 0)[0]
        assert np.array_equal(got, ref_table(h[0], STRETCH, clip_lo, 0))
        assert (got[:lo + 1] == 0).all() and got[lo + 1] > 0, clip_lo
    for clip_hi, hi in ((59, 240), (60, 30), (61, 30)):                   # N - c(239) == k_hi + 1, == k_hi, < k_hi
        got = tables_of(pkg, L, h, STRETCH, 0, clip_hi)[0]
        assert np.array_equal(got, ref_table(h[0], STRETCH, 0, clip_hi))
        assert (got[hi:] == 255).all() and got[hi - 1] < 255, clip_hi
    # the largest clips
    for _ in range(5):
        h = rng.integers(0, 1000, size=(1, BINS)).astype(np.uint32)
        assert np.array_equal(tables_of(pkg, L, h, STRETCH, CLIP_MAX, CLIP_MAX)[0], ref_table(h[0], STRETCH, CLIP_MAX, CLIP_MAX))
    assert np.array_equal(tables_of(pkg, L, hist_of_levels({5: 1}), STRETCH, CLIP_MAX, CLIP_MAX)[0], IDENT)


def test_tables_joint_and_masks(pkg, L):
    rng = np.random.default_rng(72)
    h = rng.integers(0, 5000, size=(4, BINS)).astype(np.uint32)
    h[:, :20] = 0
    for mode in (EQUALIZE, STRETCH):
        got = tables_of(pkg, L, h, mode, joint=1, mask=7)
        assert np.array_equal(got, ref_tables(h, mode, joint=1, mask=7))
        assert np.array_equal(got[3], IDENT) and np.array_equal(got[0], got[1]) and np.array_equal(got[1], got[2])
        assert not np.array_equal(got[0], IDENT)
        got = tables_of(pkg, L, h, mode, joint=0, mask=5)
        assert np.array_equal(got, ref_tables(h, mode, joint=0, mask=5))
        assert np.array_equal(got[1], IDENT) and np.array_equal(got[3], IDENT)
        assert mode == STRETCH or not np.array_equal(got[0], got[2])         # (the stretch sees the same levels 20..255 in both)
    # four channels of a 4096 x 4096 image: N = 2^26 per channel, 2^28 summed; one channel alone holds 2^26 in one bin
    big = np.zeros((4, BINS), np.uint32)
    big[0, 7] = 1 << 26
    big[1] = (1 << 26) // BINS
    big[2, 100:228] = (1 << 26) // 128
    big[3, 255], big[3, 0] = (1 << 26) - 1, 1
    assert all(int(big[ch].astype(np.uint64).sum()) == 1 << 26 for ch in range(4))
    for mode, lo, hi in ((EQUALIZE, 0, 0), (STRETCH, 0, 0), (STRETCH, 3000, CLIP_MAX)):
        for joint in (0, 1):
            assert np.array_equal(tables_of(pkg, L, big, mode, lo, hi, joint, 0), ref_tables(big, mode, lo, hi, joint, 0)), (mode, lo, hi, joint)
    # counts at the top of 32 bits summed over four channels: 2^34 - 4 in all
    top = np.zeros((4, BINS), np.uint32)
    top[:, 3], top[:, 250] = 0xFFFFFFFF - 9, 9
    top[2, 128] = 123456
    for mode in (EQUALIZE, STRETCH):
        assert np.array_equal(tables_of(pkg, L, top, mode, joint=1), ref_tables(top, mode, joint=1))


def test_tables_random(pkg, L):
    rng = np.random.default_rng(73)
    for k in range(200):
        c = int(rng.integers(1, 5))
        h = rng.integers(0, int(rng.choice([2, 50, 100000, 1 << 32])), size=(c, BINS)).astype(np.uint32)
        if rng.integers(0, 2):                                            # sparse: most levels empty
            h[:, rng.random(BINS) < 0.8] = 0
        mode = int(rng.integers(0, 2))
        lo, hi = (int(rng.integers(0, CLIP_MAX + 1)), int(rng.integers(0, CLIP_MAX + 1))) if mode == STRETCH else (0, 0)
        joint, mask = int(rng.integers(0, 2)), int(rng.integers(0, 1 << c))
        assert np.array_equal(tables_of(pkg, L, h, mode, lo, hi, joint, mask), ref_tables(h, mode, lo, hi, joint, mask)), (k, c, mode, lo, hi, joint, mask)


def cpu_tone(pkg, L, img, tone, n_threads, with_work=True):
    a = np.ascontiguousarray(img)
    n, h, w, c = a.shape
    out = np.full(a.size + 64, 0xA5, np.uint8)
    words = n * c * BINS
    assert L.mi_blur_tone_work_bytes(c, n) == 5 * words
    work = np.full(5 * words + 16, 0xA5, np.uint8)
    pkg.check(L.mi_blur_cpu_run_tone(a.ctypes.data, out.ctypes.data, w, h, c, n, C.byref(tone), work.ctypes.data if with_work else None, n_threads),
              "mi_blur_cpu_run_tone")
    assert (out[a.size:] == 0xA5).all() and (work[5 * words:] == 0xA5).all()
    return out[:a.size].reshape(a.shape), work[:4 * words].view(np.uint32).reshape(n, c, BINS), work[4 * words:5 * words].reshape(n, c, BINS)


@pytest.mark.parametrize("c", [1, 3, 4])
def test_tone_is_the_composition(pkg, L, c):
    rng = np.random.default_rng(74 + c)
    img = rng.integers(0, 256, size=(3, 33, 47, c), dtype=np.uint8)
    img[1] = (90 + img[1] % 51).astype(np.uint8)                          # a low-contrast image: another table
    n, h, w, _ = img.shape
    for mode, lo, hi in ((EQUALIZE, 0, 0), (STRETCH, 0, 0), (STRETCH, 655, 1310)):
        for joint in (0, 1):
            for mask in (0, 1) + ((5,) if c >= 3 else ()):
                tone = pkg.Tone(mode, lo, hi, joint, mask)
                got, hist, tables = cpu_tone(pkg, L, img, tone, 3)
                want, want_hist, want_tables = ref_tone(img, mode, lo, hi, joint, mask)
                assert np.array_equal(hist, want_hist) and np.array_equal(tables, want_tables) and np.array_equal(got, want)
                assert not np.array_equal(tables[0], tables[1])
                # the three steps one by one
                step_hist = cpu_hist(pkg, L, img, 2)
                step_tables = np.stack([tables_of(pkg, L, step_hist[i], mode, lo, hi, joint, mask) for i in range(n)])
                step_out = np.full(img.size + 16, 0xA5, np.uint8)
                pkg.check(L.mi_blur_cpu_run_tables(img.ctypes.data, step_out.ctypes.data, w, h, c, n, step_tables.ctypes.data, 2), "mi_blur_cpu_run_tables")
                assert (step_out[img.size:] == 0xA5).all() and np.array_equal(step_out[:img.size].reshape(img.shape), got)
                # work = NULL: the same image
                assert np.array_equal(cpu_tone(pkg, L, img, tone, 1, with_work=False)[0], got)


def test_statuses(pkg, L):
    OK, INVALID = pkg.OK, pkg.ERR_INVALID
    a = np.zeros((8, 8, 3), np.uint8)
    b = np.zeros((8, 8, 3), np.uint8)
    hist = np.zeros(3 * BINS + 4, np.uint32)
    work = np.zeros(5 * 3 * BINS + 16, np.uint8)
    tabs = np.tile(IDENT, 3)
    ia, ib, ih, iw, it = a.ctypes.data, b.ctypes.data, hist.ctypes.data, work.ctypes.data, tabs.ctypes.data
    assert ih % 16 == 0 and iw % 16 == 0
    good = pkg.Tone(EQUALIZE, 0, 0, 0, 0)
    bad_tones = [pkg.Tone(2, 0, 0, 0, 0), pkg.Tone(-1, 0, 0, 0, 0), pkg.Tone(STRETCH, -1, 0, 0, 0), pkg.Tone(STRETCH, 0, CLIP_MAX + 1, 0, 0),
                 pkg.Tone(EQUALIZE, 1, 0, 0, 0), pkg.Tone(EQUALIZE, 0, 1, 0, 0), pkg.Tone(STRETCH, 0, 0, 2, 0), pkg.Tone(STRETCH, 0, 0, -1, 0),
                 pkg.Tone(EQUALIZE, 0, 0, 0, 8), pkg.Tone(EQUALIZE, 0, 0, 0, -1)]
    out = np.full(3 * BINS, 0xA5, np.uint8)
    for k, t in enumerate(bad_tones):
        assert L.mi_blur_tone_tables(ih, 3, C.byref(t), out.ctypes.data) == INVALID, k
        assert L.mi_blur_cpu_run_tone(ia, ib, 8, 8, 3, 1, C.byref(t), None, 1) == INVALID, k
        assert L.mi_blur_enqueue_tone(ia, ib, 8, 8, 3, 1, C.byref(t), iw, None) == INVALID, k
        assert L.mi_blur_run_tone(pkg.DEVICE_CPU, ia, ib, None, 8, 8, 3, 1, C.byref(t)) == INVALID, k
    assert (out == 0xA5).all() and not b.any()
    assert L.mi_blur_tone_tables(ih, 3, C.byref(pkg.Tone(EQUALIZE, 0, 0, 0, 4)), out.ctypes.data) == OK      # bit 2 of 3 channels
    for c in (0, 5):
        assert L.mi_blur_tone_tables(ih, c, C.byref(good), out.ctypes.data) == INVALID
        assert L.mi_blur_cpu_run_hist(ia, ih, 8, 8, c, 1, 1) == INVALID
        assert L.mi_blur_enqueue_hist(ia, ih, 8, 8, c, 1, None) == INVALID
        assert L.mi_blur_cpu_run_tables(ia, ib, 8, 8, c, 1, it, 1) == INVALID
        assert L.mi_blur_enqueue_tables(ia, ib, 8, 8, c, 1, it, None) == INVALID
        assert L.mi_blur_cpu_run_tone(ia, ib, 8, 8, c, 1, C.byref(good), None, 1) == INVALID
        assert L.mi_blur_enqueue_tone(ia, ib, 8, 8, c, 1, C.byref(good), iw, None) == INVALID
        assert L.mi_blur_run_hist(0, ia, ih, 8, 8, c, 1) == INVALID
        assert L.mi_blur_tone_work_bytes(c, 1) == 0
    # null pointers, in == out, bad sizes, a negative count
    assert L.mi_blur_tone_tables(None, 3, C.byref(good), out.ctypes.data) == INVALID
    assert L.mi_blur_tone_tables(ih, 3, None, out.ctypes.data) == INVALID
    assert L.mi_blur_tone_tables(ih, 3, C.byref(good), None) == INVALID
    for hist_call in (lambda i, h_, w=8, h=8, n=1: L.mi_blur_cpu_run_hist(i, h_, w, h, 3, n, 1),
                      lambda i, h_, w=8, h=8, n=1: L.mi_blur_enqueue_hist(i, h_, w, h, 3, n, None),
                      lambda i, h_, w=8, h=8, n=1: L.mi_blur_run_hist(pkg.DEVICE_CPU, i, h_, w, h, 3, n),
                      lambda i, h_, w=8, h=8, n=1: L.mi_blur_run_hist(0, i, h_, w, h, 3, n)):
        assert hist_call(None, ih) == INVALID and hist_call(ia, None) == INVALID
        assert hist_call(ia, ih, w=0) == INVALID and hist_call(ia, ih, h=-1) == INVALID and hist_call(ia, ih, n=-1) == INVALID
        assert hist_call(ia, ih, w=32769, h=1) == INVALID and hist_call(ia, ih, w=32768, h=32768) == INVALID
        assert hist_call(ia, ih, n=0) == OK
    for apply_call in (lambda i, o, t=it, n=1, w=8: L.mi_blur_cpu_run_tables(i, o, w, 8, 3, n, t, 1),
                       lambda i, o, t=it, n=1, w=8: L.mi_blur_enqueue_tables(i, o, w, 8, 3, n, t, None),
                       lambda i, o, t=iw, n=1, w=8: L.mi_blur_cpu_run_tone(i, o, w, 8, 3, n, C.byref(good), t, 1),
                       lambda i, o, t=iw, n=1, w=8: L.mi_blur_enqueue_tone(i, o, w, 8, 3, n, C.byref(good), t, None),
                       lambda i, o, t=iw, n=1, w=8: L.mi_blur_run_tone(pkg.DEVICE_CPU, i, o, t, w, 8, 3, n, C.byref(good)),
                       lambda i, o, t=iw, n=1, w=8: L.mi_blur_run_tone(0, i, o, t, w, 8, 3, n, C.byref(good))):
        assert apply_call(None, ib) == INVALID and apply_call(ia, None) == INVALID and apply_call(ia, ia) == INVALID
        assert apply_call(ia, ib, n=-1) == INVALID and apply_call(ia, ib, w=0) == INVALID
        assert apply_call(ia, ib, n=0) == OK
    assert L.mi_blur_cpu_run_tables(ia, ib, 8, 8, 3, 1, None, 1) == INVALID
    assert L.mi_blur_enqueue_tables(ia, ib, 8, 8, 3, 1, None, None) == INVALID
    assert L.mi_blur_enqueue_tone(ia, ib, 8, 8, 3, 1, C.byref(good), None, None) == INVALID
    assert L.mi_blur_cpu_run_tone(ia, ib, 8, 8, 3, 1, None, None, 1) == INVALID
    # misaligned d_hist / d_work
    for off in (4, 8, 12):
        assert L.mi_blur_enqueue_hist(ia, ih + off, 8, 8, 3, 1, None) == INVALID
        assert L.mi_blur_enqueue_tone(ia, ib, 8, 8, 3, 1, C.byref(good), iw + off, None) == INVALID
    assert L.mi_blur_cpu_run_hist(ia, ih + 2, 8, 8, 3, 1, 1) == INVALID
    assert L.mi_blur_cpu_run_tone(ia, ib, 8, 8, 3, 1, C.byref(good), iw + 1, 1) == INVALID
    assert not b.any() and not hist.any() and not work.any()
    if L.mi_blur_device_count() <= 0:
        assert L.mi_blur_run_hist(0, ia, ih, 8, 8, 3, 1) == pkg.ERR_NO_DEVICE
        assert L.mi_blur_run_tone(0, ia, ib, None, 8, 8, 3, 1, C.byref(good)) == pkg.ERR_NO_DEVICE
        assert L.mi_blur_enqueue_hist(ia, ih, 8, 8, 3, 1, None) == pkg.ERR_NO_DEVICE
        assert L.mi_blur_enqueue_tables(ia, ib, 8, 8, 3, 1, it, None) == pkg.ERR_NO_DEVICE
        assert L.mi_blur_enqueue_tone(ia, ib, 8, 8, 3, 1, C.byref(good), iw, None) == pkg.ERR_NO_DEVICE
    assert L.mi_blur_run_hist(99, ia, ih, 8, 8, 3, 1) == pkg.ERR_NO_DEVICE and L.mi_blur_run_hist(-2, ia, ih, 8, 8, 3, 1) == pkg.ERR_NO_DEVICE
    assert L.mi_blur_version() == 1


def test_blocking_exports_and_numpy_functions_on_the_cpu_device(pkg, L):
    rng = np.random.default_rng(75)
    cpu = pkg.DEVICE_CPU
    stack = rng.integers(0, 256, size=(5, 18, 26, 3), dtype=np.uint8)
    stack[2] = (60 + stack[2] % 100).astype(np.uint8)
    n, h, w, c = stack.shape
    hist = np.full((n, c, BINS), 7, np.uint32)
    assert L.mi_blur_run_hist(cpu, stack.ctypes.data, hist.ctypes.data, w, h, c, n) == pkg.OK
    assert np.array_equal(hist, ref_hist(stack))
    assert np.array_equal(pkg.histogram(stack, device=cpu), ref_hist(stack))
    assert np.array_equal(pkg.histogram(stack, device=cpu, batch=2), ref_hist(stack))
    assert pkg.histogram(stack[1], device=cpu).shape == (3, BINS) and np.array_equal(pkg.histogram(stack[1], device=cpu), ref_hist(stack[1:2])[0])
    grey = np.ascontiguousarray(stack[0, :, :, 1])
    assert np.array_equal(pkg.histogram(grey, device=cpu), ref_hist(grey[None, :, :, None])[0])
    # tone_tables(): one image and a stack, every argument
    assert np.array_equal(pkg.tone_tables(hist[0]), ref_tables(hist[0], EQUALIZE))
    got = pkg.tone_tables(hist, "stretch", clip=(300, 900), joint=True, channels=(0, 2))
    assert got.shape == hist.shape and got.dtype == np.uint8
    assert all(np.array_equal(got[i], ref_tables(hist[i], STRETCH, 300, 900, 1, 5)) for i in range(n))
    # equalize_hist() in its three modes
    assert np.array_equal(pkg.equalize_hist(stack, device=cpu), ref_tone(stack, EQUALIZE)[0])
    assert np.array_equal(pkg.equalize_hist(stack, "joint", device=cpu, batch=2), ref_tone(stack, EQUALIZE, joint=1)[0])
    ycc = ref_preset(stack, "rgb2ycbcr")
    want = ref_preset(ref_tone(ycc, EQUALIZE, mask=1)[0], "ycbcr2rgb")
    assert np.array_equal(pkg.equalize_hist(stack, "luma", device=cpu, batch=3), want)
    assert np.array_equal(pkg.equalize_hist(stack[2], "luma", device=cpu), want[2])
    assert np.array_equal(pkg.equalize_hist(grey, device=cpu), ref_tone(grey[None, :, :, None], EQUALIZE)[0][0, :, :, 0])
    # auto_levels(): fractions to Q16 with floor
    assert np.array_equal(pkg.auto_levels(stack, device=cpu), ref_tone(stack, STRETCH, joint=1)[0])
    q = lambda f: int(np.floor(f * 65536))
    assert np.array_equal(pkg.auto_levels(stack, 0.01, device=cpu, batch=2), ref_tone(stack, STRETCH, q(0.01), q(0.01), 1)[0])
    assert np.array_equal(pkg.auto_levels(stack, (0.02, 0.1), joint=False, channels=(1,), device=cpu), ref_tone(stack, STRETCH, q(0.02), q(0.1), 0, 2)[0])
    low = pkg.auto_levels(stack[2], device=cpu)
    assert low.min() == 0 and low.max() == 255 and stack[2].min() == 60
    for bad in (lambda: pkg.equalize_hist(stack, "luminance", device=cpu), lambda: pkg.equalize_hist(stack[..., :2], "luma", device=cpu),
                lambda: pkg.auto_levels(stack, 0.5, device=cpu), lambda: pkg.auto_levels(stack, -0.1, device=cpu),
                lambda: pkg.auto_levels(stack, channels=(3,), device=cpu), lambda: pkg.histogram(np.zeros((2, 4, 4, 5), np.uint8), device=cpu),
                lambda: pkg.histogram(stack.astype(np.float32), device=cpu), lambda: pkg.tone_tables(hist, "gamma"),
                lambda: pkg.tone_tables(np.zeros((5, BINS), np.uint32))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(pkg.MiBlurError):
        pkg.tone_tables(hist, "equalize", clip=(1, 0))


def test_constants_and_no_scratch(pkg, tmp_path):
    """hist_ref.py's copies of the kernels' units, and the tiled kernels compiled to gfx950 assembly (no GPU needed):
    four instances each, none spills or indexes registers at run time."""
    text = open(os.path.join(pkg.CSRC, "filter.h")).read()
    assert f"constexpr int COLOR_GROUP = {GROUP};" in text and f"constexpr int HIST_RUN = {RUN};" in text
    assert f"constexpr int HIST_IMAGE_BLOCKS = {IMAGE_BLOCKS};" in text
    assert "#define MI_BLUR_HIST_BINS 256" in open(pkg.HEADER).read() and pkg.HIST_BINS == BINS
    no_scratch(pkg, tmp_path, "hist_kernels.hip", "blur_hist_tiled_kernel", 4)
    no_scratch(pkg, tmp_path, "hist_kernels.hip", "blur_tables_tiled_kernel", 4)


@needs_gxx
def test_hist_clean_under_asan_ubsan(pkg, tmp_path):
    run_sanitized(pkg, tmp_path, ("san_hist.cpp", "cpu_device.cpp"), ["tile geometry clean", "hist and tables cases clean", "extreme histograms clean"])
