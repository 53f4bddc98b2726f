"""The reference helpers of tests/test_grid_caps_gpu.py and tests/test_large_shapes_newer_gpu.py against the restatements
they shorten, on images small enough for those (no GPU): the area resize from prefix sums, the remap from a slab of input
rows, the rows of an integral image without the table, and the arithmetic that puts the shapes of the grid-cap tests past
their caps and outside every fast path."""
import numpy as np
import pytest

import large_harness as lh
from area_ref import MAX_RATIO, ref_area, ref_area_rows, ref_axis
from box_ref import ref_integral, ref_integral_rows
from remap_ref import BILINEAR, CLAMP, CONSTANT, NEAREST, ONE, build_map, identity_map, map_rows, ref_remap, ref_remap_slab

# the shapes and the targets of tests/test_area_host.py, restated
AREA_SHAPES = [(3, 33, 40, 3), (1, 1, 1, 3), (2, 9, 5, 1), (1, 17, 16, 4), (1, 50, 7, 5), (1, 64, 96, 2)]


def area_targets(h, w):
    return [(w, h), (-(-w // 2), -(-h // 2)), (max(1, round(0.6 * w)), max(1, round(0.6 * h))), (-(-w // MAX_RATIO), -(-h // MAX_RATIO)), (max(1, w - 1), max(1, h - 3)),
            (2 * w, 2 * h), (w + (w + 1) // 2, max(1, h // 2)), (max(1, w // 3), 2 * h + 1)]


@pytest.mark.parametrize("shape", AREA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_area_rows_equal_the_restatement(shape):
    """Whole, and in bands of up to 4 output rows from the slab i_lo(Y0) .. i_hi(Y1 - 1) alone."""
    n, h, w, c = shape
    img = np.random.default_rng(sum(shape)).integers(0, 256, size=shape, dtype=np.uint8)
    for wo, ho in area_targets(h, w):
        want = ref_area(img, wo, ho)
        assert np.array_equal(ref_area_rows(img, 0, h, wo, ho, (0, ho)), want), (wo, ho)
        i_lo, i_hi, _, _ = ref_axis(h, ho)
        for Y0 in sorted({0, ho // 2, max(ho - 4, 0)}):
            Y1 = min(Y0 + 4, ho)
            lo, hi = int(i_lo[Y0]), int(i_hi[Y1 - 1]) + 1
            assert np.array_equal(ref_area_rows(img[:, lo:hi], lo, h, wo, ho, (Y0, Y1)), want[:, Y0:Y1]), (wo, ho, Y0)


def test_area_rows_hold_at_the_largest_axis():
    """32768 -> 512 along a row, where the weight matrix of ref_area would have 16 M entries: every output is the mean of
    its 2 x 64 inputs, rounded half up."""
    img = np.random.default_rng(5).integers(0, 256, size=(1, 2, 32768, 1), dtype=np.uint8)
    s = img.astype(np.int64).reshape(1, 2, 512, 64).sum(axis=(1, 3))
    assert np.array_equal(ref_area_rows(img, 0, 2, 512, 1, (0, 1))[:, 0, :, 0], (2 * s + 128) // 256)


@pytest.mark.parametrize("border", [CLAMP, CONSTANT], ids=["clamp", "constant"])
@pytest.mark.parametrize("mode", [BILINEAR, NEAREST], ids=["bilinear", "nearest"])
def test_remap_slab_equals_the_restatement(mode, border):
    """Bands of output rows at the top, in the middle and at the bottom of maps that read beyond the image on every side:
    from the slab map_rows() names, and from a slab two rows larger where the image has them."""
    n, h, w, c = 2, 61, 40, 3
    wo, ho = 48, 57
    img = np.random.default_rng(9).integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    maps = [build_map(name, w, h, wo, ho) for name in ("rot30", "subpixel", "extremes")]
    maps.append(identity_map(wo, ho, -5 * ONE // 8, 3 * ONE + ONE // 3))          # runs off the bottom
    seen_inside = 0
    for fmap in maps:
        want = ref_remap(img, fmap, mode, border, 173)
        for Y0 in (0, 24, ho - 8):
            band = fmap[Y0:Y0 + 8]
            lo, hi = map_rows(band, mode, w, h)
            for grow in (0, 2):
                a, b = max(lo - grow, 0), min(hi + 1 + grow, h)
                seen_inside += a > 0 and b < h
                assert np.array_equal(ref_remap_slab(img[:, a:b], a, h, band, mode, border, 173), want[:, Y0:Y0 + 8]), (Y0, grow)
    assert seen_inside >= 4                                                      # slabs that end inside the image at both ends occurred


def test_integral_rows_equal_the_table():
    img = np.random.default_rng(10).integers(0, 256, size=(300, 301, 2), dtype=np.uint8)
    img[40:] = 255                                                              # Q passes 2^32 within the last rows
    starts = (0, 5, 64, 71, 292)
    for square in (False, True):
        want = ref_integral(img[None], square)[0]
        assert not square or (img[..., 0].astype(np.int64) ** 2).sum() > 1 << 32
        for chunk in (64, 7, 1000):
            got = ref_integral_rows(img, starts, 8, square, chunk)
            assert sorted(got) == sorted(starts)
            for r in starts:
                assert got[r].dtype == np.uint32 and np.array_equal(got[r], want[r:r + 8]), (square, chunk, r)


def test_the_grid_cap_shapes_are_past_their_caps():
    """The caps, restated from csrc/kernel_common.h, csrc/integral_kernels.hip and csrc/hist_kernels.hip."""
    lh.check_past_the_caps(16384 * 256, 65536 * 4, 256, 64 * 512)
    n, h, w, c = lh.BASE
    bands = lh.bands_of(lh.BASE, (16384 * 256, 2 * 16384 * 256))
    assert bands == [(0, 0), (1, 521), (2, h - 8)]
    for (i, r0), byte in zip(bands[1:], (16384 * 256, 2 * 16384 * 256)):
        first = (i * h + r0) * w * c
        assert first <= byte < first + 8 * w * c                                # the band holds the byte it is there for
    # one thread per pixel: pixel 2 * CAP of the 9 grey images lies in the last image
    assert lh.bands_of((9, h, w, 3), (16384 * 256, 2 * 16384 * 256), 3) == [(0, 0), (4, 520), (8, h - 8)]
