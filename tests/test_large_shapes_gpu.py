"""Large and extreme shapes on a real MI355X (-m gpu) for the eight families beside the box blur (sep, median, morph,
bilateral, conv, sep_down, resize, warp): one-row, one-column, very wide and very tall frames, resize and warp at
MI_BLUR_RESIZE_MAX_DIM, and one image within 75 kB of 2^31 bytes (for the warp on either side).  What is under test is the
offset arithmetic: strips times tile rows in the thousands, strips cut from 16384 chunks per row, source row times pitch
past 2^30 and near 2^31, and for the warp Q16 positions at and past 2^31.  Byte for byte against
the numpy restatements; at the largest radii, where those take too long on these frames, against the library's CPU device
(which test_*_host.py tie to the same restatements), as each case says."""
import ctypes as C

import numpy as np
import pytest

import conv_ref as cr
from filter_harness import BILATERAL, CONV, MEDIAN, MORPH, SEP, cpu_run, gpu_run, torch_cuda  # noqa: F401
from morph_ref import GRADIENT
import resample_harness as rh
from resize_ref import BILINEAR, MAX_DIM, NEAREST, ref_axis, ref_resize, takes_tiled
from sep_down_ref import ref_sep_down
from sep_ref import rand_taps
import warp_ref as wr

pytestmark = pytest.mark.gpu

CPU_THREADS = 16
DOWN_TILED, DOWN_GENERIC = "blur_sep_down_tiled_kernel", "blur_sep_down_generic_kernel"
RESIZE_TILED, RESIZE_GENERIC = "blur_resize_tiled_kernel", "blur_resize_generic_kernel"
WARP_TILED, WARP_GENERIC = "blur_warp_tiled_kernel", "blur_warp_generic_kernel"

# (h, w, c): one row; one column; 16384 chunks per row (512 strips); one chunk per row and 2188 tile rows; a ragged row of a
# million pixels; 6 chunks per row and one row more than 2^16
EXTREME = [(1, 100000, 3), (100000, 1, 3), (3, 65536, 4), (70000, 16, 1), (2, 1000003, 1), (65537, 48, 2)]


def shape_id(s):
    return "x".join(map(str, s))


def aligned(h, w, c):
    return w * c % 16 == 0 and c <= 4


# family -> (its record, (filter at a small radius, filter at its largest radius), whether numpy is the reference at the largest)
def family_filters(pkg, name, rng):
    if name == "sep":
        return SEP, [pkg.SepKernel.from_taps(rand_taps(rng, r), rand_taps(rng, r)) for r in (1, pkg.SEP_MAX_RADIUS)], False
    if name == "median":
        return MEDIAN, [1, pkg.MEDIAN_MAX_RADIUS], False
    if name == "morph":
        return MORPH, [(GRADIENT, 1, 1), (GRADIENT, pkg.MORPH_MAX_RADIUS, pkg.MORPH_MAX_RADIUS)], True
    if name == "bilateral":
        return BILATERAL, [pkg.Bilateral.gauss(0.0, 25.0, r) for r in (1, pkg.BILATERAL_MAX_RADIUS)], False
    r = pkg.CONV_MAX_RADIUS
    return CONV, [cr.make_kernel(pkg, **cr.random_kernel(rng, 1, 1, mode="sat")), cr.make_kernel(pkg, **cr.random_kernel(rng, r, r, mode="mag"))], False


FAMILIES = ("sep", "median", "morph", "bilateral", "conv")


@pytest.fixture(scope="module")
def extreme_images():
    rng = np.random.default_rng(404)
    out = {}
    for shape in EXTREME:
        img = rng.integers(0, 256, size=(1,) + shape, dtype=np.uint8)
        img.setflags(write=False)
        out[shape] = img
    return out


@pytest.mark.parametrize("shape", EXTREME, ids=shape_id)
@pytest.mark.parametrize("family", FAMILIES)
def test_extreme_aspect_ratios(pkg, L, torch_cuda, extreme_images, family, shape):
    """One launch at a small radius against the numpy restatement, one at the largest radius against the CPU device
    (morph: numpy at both, its restatement is quick)."""
    fam, filters, numpy_at_largest = family_filters(pkg, family, np.random.default_rng(sum(shape)))
    img = extreme_images[shape]
    for k, filt in enumerate(filters):
        want = fam.ref(img, filt) if k == 0 or numpy_at_largest else cpu_run(fam, pkg, L, img, filt, CPU_THREADS, prefill=False)
        got = gpu_run(fam, pkg, L, torch_cuda, img.copy(), filt, offset_out=64)     # the shared image is read-only
        assert L.mi_blur_last_kernel().decode() == fam.kernel(filt, aligned(*shape)), (family, shape, k)
        assert np.array_equal(got, want), (family, shape, k)


@pytest.mark.parametrize("shape", [s for s in EXTREME if s[0] >= 2 and s[1] >= 2], ids=shape_id)
def test_extreme_aspect_ratios_sep_down(pkg, L, torch_cuda, extreme_images, shape):
    """Stride 2 x 2, phases (0, 0) and (1, 1): radius 2 against the numpy restatement, radius 16 against the CPU device."""
    rng = np.random.default_rng(sum(shape))
    img = extreme_images[shape]
    h, w, c = shape
    kernel = DOWN_TILED if w * c % 32 == 0 else DOWN_GENERIC
    for r in (2, pkg.SEP_MAX_RADIUS):
        wx, wy = rand_taps(rng, r), rand_taps(rng, r)
        k = pkg.SepKernel.from_taps(wx, wy)
        for dec in ((2, 2, 0, 0), (2, 2, 1, 1)):
            want = ref_sep_down(img, wx, wy, *dec) if r == 2 else rh.cpu_run(rh.SEP_DOWN, pkg, L, img, (k, dec), CPU_THREADS)
            got = rh.gpu_run(rh.SEP_DOWN, pkg, L, torch_cuda, img.copy(), (k, dec), offset_out=64)
            assert L.mi_blur_last_kernel().decode() == kernel, (shape, r, dec)
            assert np.array_equal(got, want), (shape, r, dec)


# (input h, w, c), output width, output height: to and from MI_BLUR_RESIZE_MAX_DIM on either axis
RESIZE_EXTREME = [((1, 16, 1), MAX_DIM, 1), ((16, 1, 3), 1, MAX_DIM), ((2, MAX_DIM, 1), MAX_DIM, 3), ((3, 65536 // 4, 4), MAX_DIM, 3),
                  ((2, MAX_DIM, 1), 12345, 1)]


@pytest.mark.parametrize("case", RESIZE_EXTREME, ids=lambda c: shape_id(c[0]) + f"-{c[1]}x{c[2]}")
def test_extreme_aspect_ratios_resize(pkg, L, torch_cuda, case):
    shape, wo, ho = case
    assert max(shape[0], shape[1], wo, ho) == MAX_DIM
    img = np.random.default_rng(wo + ho).integers(0, 256, size=(1,) + shape, dtype=np.uint8)
    for mode in (BILINEAR, NEAREST):
        got = rh.gpu_run(rh.RESIZE, pkg, L, torch_cuda, img, (wo, ho, mode), offset_out=64)
        assert L.mi_blur_last_kernel().decode() == (RESIZE_TILED if takes_tiled(img.shape, wo, ho, mode, 0, 64) else RESIZE_GENERIC), (case, mode)
        assert np.array_equal(got, ref_resize(img, wo, ho, mode)), (case, mode)
    d = torch_cuda.zeros(64, dtype=torch_cuda.uint8, device="cuda")  # never touched: one past the limit on either side is refused up front
    r = pkg.Resize(MAX_DIM + 1, ho, BILINEAR)
    assert L.mi_blur_enqueue_resize(d.data_ptr(), d.data_ptr() + 32, shape[1], shape[0], shape[2], 1, C.byref(r), None) == pkg.ERR_INVALID
    r = pkg.Resize(wo, ho, BILINEAR)
    assert L.mi_blur_enqueue_resize(d.data_ptr(), d.data_ptr() + 32, MAX_DIM + 1, shape[0], shape[2], 1, C.byref(r), None) == pkg.ERR_INVALID


@pytest.mark.parametrize("border", [wr.CLAMP, wr.CONSTANT], ids=["clamp", "constant"])
@pytest.mark.parametrize("case", wr.EXTREME, ids=wr.extreme_id)
def test_extreme_aspect_ratios_warp(pkg, L, torch_cuda, case, border):
    """32768 pixels along one axis: Q16 positions reach 2^31 and there are hundreds of strips or tile rows.  BILINEAR on the
    tiled kernel, NEAREST and an output 7 bytes off alignment on the generic one; guard bytes either side of the output."""
    shape, (wo, ho), m, quarter_turns = case
    h, w, c = shape
    assert max(h, w, wo, ho) == MAX_DIM
    img = np.random.default_rng(sum(shape)).integers(0, 256, size=(1,) + shape, dtype=np.uint8)
    assert wr.outside_share(m, BILINEAR, w, h, wo, 0, ho) < 0.16           # the reference is real pixels, not fill
    assert wr.takes_tiled(img.shape, m, wo, ho, BILINEAR, border, 0, 64) and not wr.takes_tiled(img.shape, m, wo, ho, BILINEAR, border, 0, 7)
    want = wr.ref_warp(img, m, wo, ho, BILINEAR, border, 173)
    for mode, offset_out, kernel in ((BILINEAR, 64, WARP_TILED), (NEAREST, 64, WARP_GENERIC), (BILINEAR, 7, WARP_GENERIC)):
        got = rh.gpu_run(rh.WARP, pkg, L, torch_cuda, img, (m, wo, ho, mode, border, 173), offset_out=offset_out)
        assert L.mi_blur_last_kernel().decode() == kernel, (mode, offset_out)
        assert np.array_equal(got, want if mode == BILINEAR else wr.ref_warp(img, m, wo, ho, NEAREST, border, 173)), (mode, offset_out)
        if quarter_turns is not None:
            assert np.array_equal(got, np.rot90(img, quarter_turns, axes=(1, 2))), (mode, offset_out)


# ---------------------------------------------------------------- one image near 2^31 bytes
BIG_H, BIG_W, BIG_C = 26757, 26752, 3          # 80256-byte rows: whole 32-byte pairs and whole groups of six chunks
BAND = 8
assert BIG_W * BIG_H * BIG_C < 2 ** 31 <= BIG_W * (BIG_H + 1) * BIG_C


def band_starts(h):
    """First rows of the compared bands: the top, around the 2^30-byte offset (13380 rows of 80256 bytes are just past
    it), the middle, the bottom."""
    return (0, min(13376, h - BAND), h // 2 + 5, h - BAND)


def big_random(torch, h):
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    return torch.randint(0, 256, (h, BIG_W, BIG_C), dtype=torch.uint8, device="cuda", generator=g)


def slab(d_in, lo, hi):
    return np.ascontiguousarray(d_in[lo:hi].cpu().numpy())[None]


@pytest.mark.parametrize("family", FAMILIES)
def test_single_image_near_the_2gib_limit(pkg, L, torch_cuda, family):
    """One launch at a small radius on 26757 x 26752 x 3; bands of 8 rows against the restatement of the slab of input rows
    each needs (where the slab ends inside the image it holds the filter's halo, where it touches the image's edge the
    clamp is the image's own).  One more row is refused up front."""
    torch = torch_cuda
    fam, (filt, _), _ = family_filters(pkg, family, np.random.default_rng(5))
    ry = fam.halo(filt)
    d_in = big_random(torch, BIG_H)
    d_out = torch.empty_like(d_in)
    try:
        pkg.check(fam.enqueue(L, d_in.data_ptr(), d_out.data_ptr(), BIG_W, BIG_H, BIG_C, 1, filt, None), family)
        torch.cuda.synchronize()
        assert L.mi_blur_last_kernel().decode() == fam.kernel(filt)
        for r0 in band_starts(BIG_H):
            lo, hi = max(r0 - ry, 0), min(r0 + BAND + ry, BIG_H)
            want = fam.ref(slab(d_in, lo, hi), filt)[0, r0 - lo:r0 - lo + BAND]
            assert np.array_equal(d_out[r0:r0 + BAND].cpu().numpy(), want), (family, r0)
        assert fam.enqueue(L, d_in.data_ptr(), d_out.data_ptr(), BIG_W, BIG_H + 1, BIG_C, 1, filt, None) == pkg.ERR_INVALID
    finally:
        del d_in, d_out
        torch.cuda.empty_cache()


def test_single_image_near_the_2gib_limit_sep_down(pkg, L, torch_cuda):
    """2 x 2 at phase (1, 1): output rows Y come from input rows 1 + 2 Y."""
    torch = torch_cuda
    rng = np.random.default_rng(6)
    wx, wy = rand_taps(rng, 2), rand_taps(rng, 2)
    k, dec, ry = pkg.SepKernel.from_taps(wx, wy), (2, 2, 1, 1), 2
    d = pkg.Decimation(*dec)
    ho, wo = (BIG_H - 1 + 1) // 2, (BIG_W - 1 + 1) // 2
    d_in = big_random(torch, BIG_H)
    d_out = torch.empty((ho, wo, BIG_C), dtype=torch.uint8, device="cuda")
    try:
        pkg.check(L.mi_blur_enqueue_sep_down(d_in.data_ptr(), d_out.data_ptr(), BIG_W, BIG_H, BIG_C, 1, C.byref(k), C.byref(d), None), "sep_down")
        torch.cuda.synchronize()
        assert L.mi_blur_last_kernel().decode() == DOWN_TILED
        for Y0 in (0, 3344, 6688, ho - BAND):                                          # 6688: input rows around the 2^30-byte offset
            first, last = 1 + 2 * Y0, 1 + 2 * (Y0 + BAND - 1)                          # input rows of the band's first and last output row
            lo, hi = max(first - ry, 0), min(last + 1 + ry, BIG_H)
            want = ref_sep_down(slab(d_in, lo, hi), wx, wy, *dec, rows=(Y0, Y0 + BAND), first_row=lo)[0]
            assert np.array_equal(d_out[Y0:Y0 + BAND].cpu().numpy(), want), Y0
        assert L.mi_blur_enqueue_sep_down(d_in.data_ptr(), d_out.data_ptr(), BIG_W, BIG_H + 1, BIG_C, 1, C.byref(k), C.byref(d), None) == pkg.ERR_INVALID
    finally:
        del d_in, d_out
        torch.cuda.empty_cache()


def test_single_image_near_the_2gib_limit_resize(pkg, L, torch_cuda):
    """13379 rows to 26757 at the same width: the OUTPUT is the image near 2^31 bytes."""
    torch = torch_cuda
    h = BIG_H // 2 + 1
    assert h == 13379
    d_in = big_random(torch, h)
    d_out = torch.empty((BIG_H, BIG_W, BIG_C), dtype=torch.uint8, device="cuda")
    ya, yb, _ = ref_axis(h, BIG_H)
    try:
        r = pkg.Resize(BIG_W, BIG_H, BILINEAR)
        pkg.check(L.mi_blur_enqueue_resize(d_in.data_ptr(), d_out.data_ptr(), BIG_W, h, BIG_C, 1, C.byref(r), None), "resize")
        torch.cuda.synchronize()
        assert L.mi_blur_last_kernel().decode() == RESIZE_TILED
        for Y0 in band_starts(BIG_H):
            lo, hi = int(ya[Y0]), int(yb[Y0 + BAND - 1]) + 1
            want = ref_resize(slab(d_in, lo, hi), BIG_W, BIG_H, rows=(Y0, Y0 + BAND), first_row=lo, height=h)[0]
            assert np.array_equal(d_out[Y0:Y0 + BAND].cpu().numpy(), want), Y0
        r = pkg.Resize(BIG_W, BIG_H + 1, BILINEAR)
        assert L.mi_blur_enqueue_resize(d_in.data_ptr(), d_out.data_ptr(), BIG_W, h, BIG_C, 1, C.byref(r), None) == pkg.ERR_INVALID
    finally:
        del d_in, d_out
        torch.cuda.empty_cache()


def enqueue_warp(pkg, L, torch, d_in, d_out, w, h, wp):
    return L.mi_blur_enqueue_warp(d_in, d_out, w, h, BIG_C, 1, C.byref(wp), torch.cuda.current_stream().cuda_stream)


def test_single_image_near_the_2gib_limit_warp(pkg, L, torch_cuda):
    """The OUTPUT near 2^31 bytes: 13379 rows to 26752 x 26757 under a sheared map (every tile's box differs, two corners of
    the output leave the image), bands against ref_warp_band under CONSTANT.  Then the INPUT near 2^31 bytes: 64 output rows
    read from its first rows, from the rows around the 2^30-byte offset and from its last rows and beyond them."""
    torch = torch_cuda
    h = BIG_H // 2 + 1
    m = [wr.Q, 0, 0, -655, wr.Q // 2, 133 * wr.Q]
    # on the reference only: the compared bands see real pixels
    first, last = wr.outside_share(m, BILINEAR, BIG_W, h, BIG_W, 0, BAND), wr.outside_share(m, BILINEAR, BIG_W, h, BIG_W, BIG_H - BAND, BIG_H)
    assert 0 < first < 0.5 and 0 < last < 0.5                                  # both leave the image, at opposite corners
    assert all(wr.outside_share(m, BILINEAR, BIG_W, h, BIG_W, Y0, Y0 + BAND) < 0.5 for Y0 in band_starts(BIG_H))
    assert wr.outside_share(m, BILINEAR, BIG_W, h, BIG_W, 13376, 13376 + BAND) == 0
    d_in = big_random(torch, h)
    d_out = torch.empty((BIG_H, BIG_W, BIG_C), dtype=torch.uint8, device="cuda")
    try:
        wp = wr.make_warp(pkg, m, BIG_W, BIG_H, BILINEAR, wr.CONSTANT, 173)
        pkg.check(enqueue_warp(pkg, L, torch, d_in.data_ptr(), d_out.data_ptr(), BIG_W, h, wp), "warp")
        torch.cuda.synchronize()
        assert L.mi_blur_last_kernel().decode() == WARP_TILED
        for Y0 in band_starts(BIG_H):
            want = wr.ref_warp_band(lambda lo, hi: slab(d_in, lo, hi), h, m, BIG_W, Y0, Y0 + BAND, BILINEAR, wr.CONSTANT, 173)[0]
            assert np.array_equal(d_out[Y0:Y0 + BAND].cpu().numpy(), want), Y0
        wp = wr.make_warp(pkg, m, BIG_W, BIG_H + 1, BILINEAR, wr.CONSTANT, 173)
        assert enqueue_warp(pkg, L, torch, d_in.data_ptr(), d_out.data_ptr(), BIG_W, h, wp) == pkg.ERR_INVALID
    finally:
        del d_in, d_out
        torch.cuda.empty_cache()

    ho, guard = 64, 64
    size = ho * BIG_W * BIG_C
    d_in = big_random(torch, BIG_H)
    d_out = torch.empty(size + 2 * guard, dtype=torch.uint8, device="cuda")
    try:
        for mode, kernel in ((BILINEAR, WARP_TILED), (NEAREST, WARP_GENERIC)):
            for first_row in (0, 13376, BIG_H - 60):                           # the last: output rows 60.. read past the last input row
                m = [wr.Q, 0, 3 * wr.Q // 8 + 1, 0, wr.Q, first_row * wr.Q + 5 * wr.Q // 8]
                for border in (wr.CLAMP, wr.CONSTANT):
                    d_out.fill_(0x5A)
                    wp = wr.make_warp(pkg, m, BIG_W, ho, mode, border, 173)
                    pkg.check(enqueue_warp(pkg, L, torch, d_in.data_ptr(), d_out.data_ptr() + guard, BIG_W, BIG_H, wp), "warp")
                    torch.cuda.synchronize()
                    assert L.mi_blur_last_kernel().decode() == kernel, (mode, first_row, border)
                    assert bool((d_out[:guard] == 0x5A).all()) and bool((d_out[guard + size:] == 0x5A).all()), "wrote outside the output"
                    got = d_out[guard:guard + size].reshape(ho, BIG_W, BIG_C)
                    for Y0 in (0, 28, ho - BAND):                              # 28: across the two tile rows
                        want = wr.ref_warp_band(lambda lo, hi: slab(d_in, lo, hi), BIG_H, m, BIG_W, Y0, Y0 + BAND, mode, border, 173)[0]
                        assert np.array_equal(got[Y0:Y0 + BAND].cpu().numpy(), want), (mode, first_row, border, Y0)
        assert 0 < wr.outside_share(m, BILINEAR, BIG_W, BIG_H, BIG_W, ho - BAND, ho) < 1       # the last band runs off the bottom
        wp = wr.make_warp(pkg, m, BIG_W, ho, BILINEAR, wr.CONSTANT, 173)
        assert enqueue_warp(pkg, L, torch, d_in.data_ptr(), d_out.data_ptr() + guard, BIG_W, BIG_H + 1, wp) == pkg.ERR_INVALID
    finally:
        del d_in, d_out
        torch.cuda.empty_cache()
