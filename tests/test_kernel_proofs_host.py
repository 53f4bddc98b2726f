"""CPU-only half of the kernel proofs (see kernel_proofs.py): the de Bruijn generator the median proof rests on, and the
CPU device (mi_blur_cpu_run_median, mi_blur_cpu_run_sep) on the same pattern sets and one-hot taps as the GPU module.
The CPU median is a sliding histogram, not a min / max network, so for it these are coverage tests, not a proof; they
tie both devices to one definition, and the count reference to an implementation other than the GPU's."""
import ctypes as C
import os

import numpy as np

import kernel_proofs as kp

N_THREADS = min(16, os.cpu_count() or 1)


def cpu_median(pkg, L, img, r):
    a = np.ascontiguousarray(img)
    out = np.full_like(a, 0xA5)
    n, h, w, c = a.shape
    pkg.check(L.mi_blur_cpu_run_median(a.ctypes.data, out.ctypes.data, w, h, c, r, n, N_THREADS), "mi_blur_cpu_run_median")
    return out


def test_debruijn_small_known():
    assert "".join(map(str, kp.debruijn(1, 3))) == "00010111"
    assert "".join(map(str, kp.debruijn(1, 5))) == "00000100011001010011101011011111"


def test_debruijn_every_window_exactly_once():
    """The proof rests on this: every run of D column values occurs exactly once in the linear sequence."""
    for m, n in ((3, 3), (5, 5), (2, 5), (4, 3)):
        seq = kp.debruijn(m, n)
        assert seq.dtype == np.uint8 and len(seq) == 1 << (m * n) and int(seq.max()) == (1 << m) - 1
        counts = np.bincount(kp.window_codes(seq, m, n), minlength=1 << (m * n))
        assert len(counts) == 1 << (m * n) and counts.min() == 1 and counts.max() == 1, (m, n)


def test_patterns_cover_every_window():
    """Every interior row of the stream image and the edge columns of the edge batch see every two-valued window."""
    r, d = 1, 3
    seq = kp.debruijn(d, d)
    for c in range(1, 5):
        m = kp.stream_mask_np(seq, r, c, 0)
        for ch in range(c):
            for y in range(r, m.shape[1] - r):
                code = np.zeros(m.shape[2] - 2 * r, np.int64)
                for j in range(d):
                    for i in range(d):
                        code = (code << 1) | m[0, y - r + j, i:i + len(code), ch]
                assert np.bincount(code, minlength=1 << (d * d)).min() >= 1, (c, ch, y)
        e = kp.edge_mask_np(r, c)
        for ch in range(c):
            for cols in (slice(0, 2 * r), slice(-2 * r, None)):
                codes = np.zeros(len(e), np.int64)
                for y in range(r, r + d):
                    for x in range(2 * r):
                        codes = (codes << 1) | e[:, y, cols, ch][:, x]
                assert len(np.unique(codes)) == kp.edge_combos(r), (c, ch, cols)


def test_count_reference_matches_the_partition_reference():
    rng = np.random.default_rng(3)
    for r in (1, 2, 3):
        mask = (rng.random((3, 9, 14, 2)) < 0.5).astype(np.uint8)
        for lo, hi in kp.MEDIAN_PAIRS:
            want = kp.ref_median(kp.two_valued(mask, lo, hi), r)
            assert np.array_equal(kp.median_from_count(kp.high_count_np(mask, r), r, lo, hi), want), r


def test_cpu_median_r1_full_pattern_set(pkg, L):
    r = 1
    seq = kp.debruijn(3, 3)
    for c in range(1, 5):
        for mask in (kp.stream_mask_np(seq, r, c, 0), kp.edge_mask_np(r, c)):
            cnt = kp.high_count_np(mask, r)
            for lo, hi in kp.MEDIAN_PAIRS:
                img = kp.two_valued(mask, lo, hi)
                want = kp.median_from_count(cnt, r, lo, hi)
                assert np.array_equal(want, kp.ref_median(img, r)), c
                assert np.array_equal(cpu_median(pkg, L, img, r), want), (c, lo, hi)


def test_cpu_median_r2_interior_stream(pkg, L):
    """B(32, 5) at one shift, one channel: 2^25 windows, cut into images that overlap by 2r columns so threads share it."""
    r, n_img = 2, 16
    seq = kp.debruijn(5, 5)
    seg = len(seq) // n_img
    mask = np.concatenate([kp.stream_mask_np(seq, r, 1, 0, x0=i * seg, w=seg + 2 * r) for i in range(n_img)])
    lo, hi = kp.MEDIAN_PAIRS[0]
    want = kp.median_from_count(kp.high_count_np(mask, r), r, lo, hi)
    got = cpu_median(pkg, L, kp.two_valued(mask, lo, hi), r)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{len(bad)} outputs differ, first at {bad[0].tolist()}"


def test_cpu_median_r2_edge_batch(pkg, L):
    """Every combination of the first and last 2r columns (32^4 of each), one and two channels."""
    r = 2
    for c in (1, 2):
        mask = kp.edge_mask_np(r, c)
        lo, hi = kp.MEDIAN_PAIRS[c - 1]
        want = kp.median_from_count(kp.high_count_np(mask, r), r, lo, hi)
        got = cpu_median(pkg, L, kp.two_valued(mask, lo, hi), r)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"C={c}: {len(bad)} outputs differ, first at {bad[0].tolist()}"


def test_cpu_sep_one_hot_taps(pkg, L):
    """A tap 2^b at offset d (every d of every radius bucket, each axis) moves the image by d pixels, clamped."""
    rng = np.random.default_rng(11)
    imgs = {}
    for c, axis, rb, d, b, w, h in kp.one_hot_cases():
        img = imgs.setdefault((c, w, h), rng.integers(0, 256, size=(1, h, w, c), dtype=np.uint8))
        t = kp.one_hot(rb, d, b)
        wx, wy = (t, [1]) if axis == 2 else ([1], t)
        k = pkg.SepKernel.from_taps(wx, wy)
        out = np.full_like(img, 0xA5)
        pkg.check(L.mi_blur_cpu_run_sep(img.ctypes.data, out.ctypes.data, w, h, c, 1, C.byref(k), 2), "mi_blur_cpu_run_sep")
        want = kp.shifted(img, d, axis)
        assert np.array_equal(want, kp.ref_sep(img, wx, wy)), (c, axis, rb, d, b)
        assert np.array_equal(out, want), (c, axis, rb, d, b, w)
