"""CPU-only half of the kernel proofs (see kernel_proofs.py): the de Bruijn generator the median proof rests on, and the
CPU device (mi_blur_cpu_run_median, mi_blur_cpu_run_sep) on the same pattern sets and one-hot taps as the GPU module.
The CPU median is a sliding histogram, not a min / max network, so for it these are coverage tests, not a proof; they
tie both devices to one definition, and the count reference to an implementation other than the GPU's.

The morph proof (kernel_proofs.py, morph_ref.py): that the proof images witness every window position anything can
witness, that the check notices weakened images, and the CPU device on the same images."""
import ctypes as C
import os

import numpy as np

import kernel_proofs as kp
import morph_ref as mr
from filter_harness import MORPH, cpu_run

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


# ---------------------------------------------------------------- the morph proof images
def proof_image(axis, c, **kw):
    return mr.proof_horizontal(c, **kw) if axis == 2 else mr.proof_vertical(c, **kw)


def test_morph_proof_images_witness_every_window_position():
    """Each of the four value pairs on its own: a window without offset d, for every d of [-r, r], and a window with the
    tap r+1 or -(r+1) added, differs from the true one at every byte column (horizontal image) or row (vertical image)
    whose clamped source for d no other offset of the window reaches.  That is the only exclusion."""
    for axis in (2, 1):
        for c in kp.MORPH_PROOF_C:
            img = proof_image(axis, c)
            assert img.shape[1:] == ((mr.PROOF_PERIOD * c, mr.PROOF_H_WIDTH, c) if axis == 2 else mr.PROOF_V_SHAPE + (c,))
            assert img.shape[2] * c % 16 == 0 and len(img) == len(mr.PROOF_PAIRS)
            for r in (1, 4, 16):
                assert kp.morph_window_gaps(img, axis, r) == [], (axis, c, r)


def test_morph_sufficiency_check_notices_weakened_images():
    """One row of the horizontal image without its impulses, and a period of 33 (a window of 33 then always holds an
    impulse, so a tap too many shows nowhere), on either image: the check reports gaps."""
    for c in (1, 3):
        gaps = kp.morph_window_gaps(mr.proof_horizontal(c, drop_row=5 * c), 2, 16)
        assert {d for d, *_ in gaps} == set(range(-17, 18)), c                # every offset has a column whose witness was that row
        for axis in (2, 1):
            gaps = kp.morph_window_gaps(proof_image(axis, c, period=33), axis, 16)
            assert gaps and {d for d, *_ in gaps} == {-17, 17}, (axis, c)


def test_window_qualifies_excludes_only_clamped_duplicates():
    assert kp.window_qualifies(10, 2, -2).tolist() == [False, False] + [True] * 8     # x = 0, 1: offset -1 clamps to pixel 0 as well
    assert kp.window_qualifies(10, 2, 0).tolist() == [False] + [True] * 8 + [False]   # at either end the centre is also a clamped tap
    assert kp.window_qualifies(10, 2, 3).tolist() == [True] * 7 + [False] * 3         # a tap too many: pixel 9 is already the window's from x = 7 on
    assert kp.window_qualifies(3, 16, 5).tolist() == [False] * 3                      # a row narrower than the window: every source is shared


def test_cpu_morph_on_the_proof_images(pkg, L):
    """mi_blur_cpu_run_morph on both images: every radius 0..16 on the proved axis with the other at 0, all three ops."""
    for axis in (2, 1):
        for c in kp.MORPH_PROOF_C:
            img = proof_image(axis, c)
            for r in kp.MORPH_PROOF_RADII:
                rx, ry = (r, 0) if axis == 2 else (0, r)
                lo, hi = mr.ref_lo_hi(img, rx, ry)
                for op in mr.OPS:
                    got = cpu_run(MORPH, pkg, L, img, (op, rx, ry), N_THREADS)
                    assert np.array_equal(got, mr._finish(lo, hi, op)), (axis, c, op, rx, ry)
