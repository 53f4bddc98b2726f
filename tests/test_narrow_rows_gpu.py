"""Rows narrower than the halo on a real MI355X (-m gpu): the one corner of the tile staging the sep, morph, bilateral
and conv kernels share (stage_tile, kernel_common.h) that the tile-edge sweeps of their own test files do not reach.
With 1-3 chunks per row the only strip has halo chunks outside the row on BOTH sides, and the x-clamp fills them from
a row that is the whole tile.  Byte for byte against the library's CPU device.

blur_sep_down_tiled_kernel stages with the same stager and needs rows of whole chunk pairs: its narrowest rows are one and
two pairs wide, with up to 4 halo chunks outside the row on both sides at the largest radius.

blur_warp_tiled_kernel has no halo; its corner is the staged box (stage_box, warp_tap of filter.h): with one chunk per input
row (3 channels: one group of three) and 1, 2 or 33 rows, the box is the whole row or the whole image, and both the + 1 tap
and the one-pixel case of warp_tap meet the edge of the box on both sides at once.  Byte for byte against the numpy
restatement of the header."""
import numpy as np
import pytest

import conv_ref as cr
from filter_harness import BILATERAL, CONV, MORPH, SEP, cpu_run, gpu_run, torch_cuda  # noqa: F401
import resample_harness as rh
from sep_ref import rand_taps
from warp_ref import BILINEAR, CLAMP, CONSTANT, narrow_cases, ref_warp, takes_tiled

pytestmark = pytest.mark.gpu

ROWS = [(16, 1), (32, 1), (8, 2), (16, 3), (4, 4), (8, 4)]      # (w, c): 1, 2, 1, 3, 1, 2 chunks per row
HEIGHTS = (1, 33)                                                # one row; one tile and one row of the next
N = 2


@pytest.fixture(scope="module")
def images():
    """(w, c, h) -> N x h x w x c random bytes with 0 / 255 impulses in the first and the last pixel of every row."""
    rng = np.random.default_rng(77)
    out = {}
    for w, c in ROWS:
        assert w * c % 16 == 0 and w * c // 16 <= 3
        for h in HEIGHTS:
            img = rng.integers(0, 256, size=(N, h, w, c), dtype=np.uint8)
            flip = (np.arange(N)[:, None] + np.arange(h)[None, :]) % 2 == 1
            img[:, :, 0, :] = np.where(flip, 255, 0)[:, :, None]
            img[:, :, -1, :] = np.where(flip, 0, 255)[:, :, None]
            img.setflags(write=False)
            out[w, c, h] = img
    return out


# family -> (its record, its filters at a radius, radius 1 and its largest radius)
FAMILIES = {"sep": (SEP, lambda pkg, rng, r: [pkg.SepKernel.from_taps(rand_taps(rng, r), rand_taps(rng, r))], (1, 16)),
            "morph": (MORPH, lambda pkg, rng, r: [(op, r, r) for op in (pkg.MORPH_ERODE, pkg.MORPH_DILATE, pkg.MORPH_GRADIENT)], (1, 16)),
            "bilateral": (BILATERAL, lambda pkg, rng, r: [pkg.Bilateral.gauss(0.0, 25.0, r)], (1, 8)),
            "conv": (CONV, lambda pkg, rng, r: [cr.make_kernel(pkg, **cr.random_kernel(rng, r, r, mode=mode)) for mode in ("sat", "mag")],  # one table and two
                     (1, 7))}


@pytest.mark.parametrize("family,r", [(f, r) for f, (_, _, radii) in FAMILIES.items() for r in radii])
def test_rows_narrower_than_the_halo(pkg, L, torch_cuda, images, family, r):
    fam, filters, radii = FAMILIES[family]
    assert radii[1] == {"sep": pkg.SEP_MAX_RADIUS, "morph": pkg.MORPH_MAX_RADIUS, "bilateral": pkg.BILATERAL_MAX_RADIUS,
                        "conv": pkg.CONV_MAX_RADIUS}[family]
    rng = np.random.default_rng(1000 + r)
    for filt in filters(pkg, rng, r):
        for (w, c, h), img in images.items():
            want = cpu_run(fam, pkg, L, img, filt, 8, prefill=False)
            got = gpu_run(fam, pkg, L, torch_cuda, img.copy(), filt, offset_out=64)     # 64 guard bytes either side
            assert L.mi_blur_last_kernel().decode() == fam.fast, (w, c, h)
            assert np.array_equal(got, want), (w, c, h)


DOWN_ROWS = [(32, 1), (16, 2), (8, 4), (16, 4), (32, 3)]         # (w, c): 2, 2, 2, 4 and 6 chunks per row (3 channels: one group of three pairs)
DOWN_HEIGHTS = (1, 2, 33)


@pytest.mark.parametrize("r", [1, 16])
def test_sep_down_rows_narrower_than_the_halo(pkg, L, torch_cuda, r):
    """Stride 2 x 2 at all four phases (one-row images: oy = 0 only, the output is never empty)."""
    rng = np.random.default_rng(2000 + r)
    k = pkg.SepKernel.from_taps(rand_taps(rng, r), rand_taps(rng, r))
    for w, c in DOWN_ROWS:
        assert w * c % 32 == 0 and w * c // 16 <= 6
        for h in DOWN_HEIGHTS:
            img = rng.integers(0, 256, size=(N, h, w, c), dtype=np.uint8)
            flip = (np.arange(N)[:, None] + np.arange(h)[None, :]) % 2 == 1
            img[:, :, 0, :] = np.where(flip, 255, 0)[:, :, None]
            img[:, :, -1, :] = np.where(flip, 0, 255)[:, :, None]
            for ox in (0, 1):
                for oy in (0, 1) if h > 1 else (0,):
                    dec = (2, 2, ox, oy)
                    want = rh.cpu_run(rh.SEP_DOWN, pkg, L, img, (k, dec), 8)
                    got = rh.gpu_run(rh.SEP_DOWN, pkg, L, torch_cuda, img, (k, dec), offset_out=64)       # 64 guard bytes either side
                    assert L.mi_blur_last_kernel().decode() == "blur_sep_down_tiled_kernel", (w, c, h, dec)
                    assert np.array_equal(got, want), (w, c, h, dec)


def test_warp_inputs_of_one_chunk_per_row(pkg, L, torch_cuda):
    """Three 64-pixel strips and two tile rows of output from inputs 16 bytes wide (48 for 3 channels), 1, 2 and 33 rows high:
    an enlargement, a rotation, a sub-pixel shift and a map wholly left of the image, under both borders."""
    for img, name, m, wo, ho in narrow_cases():
        for border in (CLAMP, CONSTANT):
            assert takes_tiled(img.shape, m, wo, ho, BILINEAR, border), (img.shape, name, border)
            got = rh.gpu_run(rh.WARP, pkg, L, torch_cuda, img, (m, wo, ho, BILINEAR, border, 173), offset_out=64)      # 64 guard bytes either side
            assert L.mi_blur_last_kernel().decode() == "blur_warp_tiled_kernel", (img.shape, name, border)
            assert np.array_equal(got, ref_warp(img, m, wo, ho, BILINEAR, border, 173)), (img.shape, name, border)
