"""Every byte-per-thread kernel past its grid cap on a real MI355X (-m gpu).  byte_grid() of csrc/kernel_common.h gives a
launch at most 16384 workgroups of 256 threads and the kernel grid-strides over the rest; the generic integral gives one
at most 65536 workgroups of 4 rows and the generic histogram gives an image at most 256 workgroups.  Every launch here is
past its cap, so the loop's stride, the image index of a later trip (one trip spans an image boundary) and whatever the
kernel set up before the loop are all in use.  Byte for byte (word for word) against the library's CPU device on the
whole output (tests/test_*_host.py tie that device to the numpy restatements), and against the family's numpy restatement
itself on three bands of 8 rows: the first rows of image 0, the rows around byte CAP and those around byte 2 CAP."""
import ctypes as C

import numpy as np
import pytest

import area_ref
import arith_ref
import box_ref
import color_ref
import conv_ref as cr
import filter_harness as fh
import hist_ref
import large_harness as lh
import remap_ref
import resample_harness as rh
import resize_ref
import warp_perspective_ref as pr
import warp_ref as wr
from color_harness import cpu_run as color_cpu_run, gpu_run as color_gpu_run, make_color
from filter_harness import torch_cuda  # noqa: F401
from large_harness import BAND, BASE
from morph_ref import GRADIENT
from sep_down_ref import ref_sep_down
from sep_ref import rand_taps

pytestmark = pytest.mark.gpu

# restated from the source, not imported from the product
CAP = 16384 * 256               # byte_grid(), csrc/kernel_common.h: workgroups x threads
ROW_CAP = 65536 * 4             # launch_integral(), csrc/integral_kernels.hip: workgroups x rows (one wave each)
HIST_PARTS = 256                # launch_hist(), csrc/hist_kernels.hip: workgroups per image ...
HIST_PART_BYTES = 64 * 512      # ... of 512 threads that take about 64 bytes each below the cap
CPU_THREADS = 16
GUARD = 64                      # the harnesses' outputs lie this far into a buffer of 0x5A with 128 bytes to spare: guards either side
N, H, W, CH = BASE
lh.check_past_the_caps(CAP, ROW_CAP, HIST_PARTS, HIST_PART_BYTES)


@pytest.fixture(scope="module")
def base():
    img = lh.own_ranges(np.random.default_rng(2201), BASE)
    img.setflags(write=False)
    return img


def compare(got, cpu, bands, band_ref, what):
    """The whole output against the CPU device, the bands against the numpy restatement."""
    assert got.shape == cpu.shape and np.array_equal(got, cpu), what
    for i, r0 in bands:
        assert np.array_equal(got[i, r0:r0 + BAND], band_ref(i, r0)), (what, i, r0)


def slab_ref(fam, img, filt):
    """The rows r0 .. r0 + 7 of image i from the slab of input rows they need: with the filter's halo where the slab ends
    inside the image; where it touches the image's edge the clamp is the image's own."""
    ry, h = fam.halo(filt), img.shape[1]

    def band(i, r0):
        lo, hi = max(r0 - ry, 0), min(r0 + BAND + ry, h)
        return fam.ref(np.ascontiguousarray(img[i:i + 1, lo:hi]), filt)[0, r0 - lo:r0 - lo + BAND]
    return band


# ---------------------------------------------------------------- the filters that keep the size
def same_size_filter(pkg, name):
    rng = np.random.default_rng(2202)
    if name == "sep":
        return fh.SEP, pkg.SepKernel.from_taps(rand_taps(rng, 2), rand_taps(rng, 2))
    if name == "median":
        return fh.MEDIAN, 1
    if name == "morph":
        return fh.MORPH, (GRADIENT, 1, 1)
    if name == "bilateral":
        return fh.BILATERAL, pkg.Bilateral.gauss(0.0, 25.0, 1)
    return fh.CONV, cr.make_kernel(pkg, **cr.random_kernel(rng, 1, 1, mode=name[5:]))


@pytest.mark.parametrize("name", ["sep", "median", "morph", "bilateral", "conv-sat", "conv-mag"])
def test_same_size_generic_kernels(pkg, L, torch_cuda, base, name):
    """blur_sep_generic_kernel (radius 2), blur_median_generic_kernel (radius 1), blur_morph_generic_kernel (GRADIENT 1 x 1),
    blur_bilateral_generic_kernel (radius 1: its tables are loaded ahead of the loop) and blur_conv_generic_kernel (3 x 3,
    "sat" and "mag": likewise) on the base shape."""
    fam, filt = same_size_filter(pkg, name)
    img = np.array(base)
    got = fh.gpu_run(fam, pkg, L, torch_cuda, img, filt, offset_out=GUARD)
    assert L.mi_blur_last_kernel().decode() == fam.generic == f"blur_{fam.name}_generic_kernel"
    cpu = fh.cpu_run(fam, pkg, L, img, filt, CPU_THREADS, prefill=False)
    compare(got, cpu, lh.bands_of(BASE, (CAP, 2 * CAP)), slab_ref(fam, img, filt), name)


BOX = fh.Family("blur", enqueue=lambda L, i, o, w, h, c, n, r, s: L.mi_blur_enqueue(i, o, w, h, c, r, n, s), enqueue_band=None,
                cpu_run=lambda L, i, o, w, h, c, n, r, nt: L.mi_blur_cpu_run(i, o, w, h, c, r, n, nt), ctx_set=None, set=None,
                fast="blur_tiled_kernel", generic="blur_generic_kernel", halo=lambda r: r, ref=None)


@pytest.mark.parametrize("radius", [1, 2])
def test_box_blur_generic_kernel(pkg, L, O, torch_cuda, base, radius):
    """blur_generic_kernel through mi_blur_enqueue.  With its default options the library gives rows that are no multiple of
    16 bytes to the ragged form of the tiled kernel, which has no capped grid; "ragged_tiled" = 0 is the documented way to
    the generic kernel for such rows (a frame of 5 to 8 channels at radius 2 takes it by default).  The restatement of the
    bands is the oracle."""
    img = np.array(base)
    fam = BOX._replace(ref=lambda slab, r: O.blur_batch(slab, r))
    try:
        assert L.mi_blur_set_option(b"ragged_tiled", 0) == pkg.OK
        got = fh.gpu_run(fam, pkg, L, torch_cuda, img, radius, offset_out=GUARD)
        assert L.mi_blur_last_kernel().decode() == "blur_generic_kernel"
    finally:
        assert L.mi_blur_set_option(b"ragged_tiled", 1) == pkg.OK
    cpu = fh.cpu_run(fam, pkg, L, img, radius, CPU_THREADS, prefill=False)
    compare(got, cpu, lh.bands_of(BASE, (CAP, 2 * CAP)), slab_ref(fam, img, radius), radius)


# (n, h, w, c): CAP - 256 and CAP + 256 outputs.  CAP - 256 = 256 * 3 * 43 * 127 and CAP + 256 = 256 * 5 * 29 * 113 share
# no odd factor, so the two launches cannot have the same row; both rows are odd, so no multiple of 16 bytes
CONTROL = {"below": (3, 11008, 127, 1), "above": (5, 7424, 113, 1)}


@pytest.mark.parametrize("side", ["below", "above"])
def test_control_either_side_of_the_cap(pkg, L, torch_cuda, side):
    """The separable filter of test_same_size_generic_kernels on a launch of 16383 workgroups, which makes one trip, and on
    one of 16385, whose first 256 threads make a second: should the tests of this file fail, this one says on which side of
    the cap the fault lies.  The bands: the first and the last rows of the launch."""
    shape = CONTROL[side]
    n, h, w, c = shape
    assert n * h * w * c == CAP + (256 if side == "above" else -256) and (w * c) % 16 != 0
    fam, filt = same_size_filter(pkg, "sep")
    img = lh.own_ranges(np.random.default_rng(2203), shape)
    got = fh.gpu_run(fam, pkg, L, torch_cuda, img, filt, offset_out=GUARD)
    assert L.mi_blur_last_kernel().decode() == "blur_sep_generic_kernel"
    cpu = fh.cpu_run(fam, pkg, L, img, filt, CPU_THREADS, prefill=False)
    compare(got, cpu, [(0, 0), (n - 1, h - BAND)], slab_ref(fam, img, filt), side)


# ---------------------------------------------------------------- the filters that change the size: BASE is the OUTPUT
def resampled(pkg, L, torch, fam, img, spec, band_ref, what):
    got = rh.gpu_run(fam, pkg, L, torch, img, spec, offset_out=GUARD)
    assert got.shape == BASE and rh.last(L) == fam.generic and not fam.takes_tiled(img.shape, spec), what
    cpu = rh.cpu_run(fam, pkg, L, img, spec, CPU_THREADS)
    compare(got, cpu, lh.bands_of(BASE, (CAP, 2 * CAP)), band_ref, what)


def test_sep_down_generic_kernel(pkg, L, torch_cuda):
    """blur_sep_down_generic_kernel: 2102 x 1774 x 3, stride 2 x 2 at phase (0, 0), radius 2."""
    rng = np.random.default_rng(2204)
    img = lh.own_ranges(rng, lh.DOWN_IN)
    wx, wy = rand_taps(rng, 2), rand_taps(rng, 2)
    dec, ry = (2, 2, 0, 0), 2

    def band(i, Y0):
        lo, hi = max(2 * Y0 - ry, 0), min(2 * (Y0 + BAND - 1) + 1 + ry, img.shape[1])
        return ref_sep_down(np.ascontiguousarray(img[i:i + 1, lo:hi]), wx, wy, *dec, rows=(Y0, Y0 + BAND), first_row=lo)[0]
    resampled(pkg, L, torch_cuda, rh.SEP_DOWN, img, (pkg.SepKernel.from_taps(wx, wy), dec), band, "sep_down")


@pytest.mark.parametrize("mode", [resize_ref.BILINEAR, resize_ref.NEAREST], ids=["bilinear", "nearest"])
def test_resize_generic_kernel(pkg, L, torch_cuda, mode):
    """blur_resize_generic_kernel: 701 x 591 x 3 to the base shape, an enlargement by no whole factor."""
    img = lh.own_ranges(np.random.default_rng(2205), lh.RESIZE_IN)
    band = lambda i, Y0: resize_ref.ref_resize(img[i:i + 1], W, H, mode, rows=(Y0, Y0 + BAND))[0]
    resampled(pkg, L, torch_cuda, rh.RESIZE, img, (W, H, mode), band, mode)


def rows_of(m, Y0):
    """The affine map m (or the homography: 9 entries) moved by Y0 output rows: its output row 0 is m's row Y0."""
    mb = list(m)
    for k in range(2, len(m), 3):
        mb[k] += m[k - 1] * Y0
    return mb


def test_warp_generic_kernel(pkg, L, torch_cuda, base):
    """blur_warp_generic_kernel: a rotation by 7 degrees about the centre, BILINEAR under CLAMP."""
    img = np.array(base)
    m = wr.rotation_m(W, H, 7.0)
    assert wr.outside_share(m, wr.BILINEAR, W, H, W, 0, H) < 0.5
    for i, Y0 in lh.bands_of(BASE, (CAP, 2 * CAP)):
        assert wr.outside_share(m, wr.BILINEAR, W, H, W, Y0, Y0 + BAND) < 0.5       # the compared bands are real pixels
    band = lambda i, Y0: wr.ref_warp(img[i:i + 1], rows_of(m, Y0), W, BAND, wr.BILINEAR, wr.CLAMP, 173)[0]
    resampled(pkg, L, torch_cuda, rh.WARP, img, (m, W, H, wr.BILINEAR, wr.CLAMP, 173), band, "warp")


def test_warp_perspective_generic_kernel(pkg, L, torch_cuda, base):
    """blur_warp_persp_generic_kernel: the refs' keystone, BILINEAR under CLAMP."""
    img = np.array(base)
    hm = pr.named_maps(W, H, W, H)["keystone"]
    assert pr.outside_share(hm, wr.BILINEAR, W, H, W, H) < 0.5
    band = lambda i, Y0: pr.ref_warp(img[i:i + 1], rows_of(hm, Y0), W, BAND, wr.BILINEAR, wr.CLAMP, 173)[0]
    for i, Y0 in lh.bands_of(BASE, (CAP, 2 * CAP)):
        assert pr.outside_share(rows_of(hm, Y0), wr.BILINEAR, W, H, W, BAND) < 0.5
    resampled(pkg, L, torch_cuda, rh.PERSP, img, (hm, W, H, wr.BILINEAR, wr.CLAMP, 173), band, "warp_perspective")


def test_remap_generic_kernel(pkg, L, torch_cuda, base):
    """blur_remap_generic_kernel: the refs' rot30 map, BILINEAR under CONSTANT."""
    img = np.array(base)
    fmap = remap_ref.build_map("rot30", W, H, W, H)
    x0, y0, _, _ = remap_ref.ref_coord(fmap[:, :, 0], fmap[:, :, 1], wr.BILINEAR, W, H)
    outside = (x0 + 1 < 0) | (x0 > W - 1) | (y0 + 1 < 0) | (y0 > H - 1)
    assert outside.mean() < 0.5
    for i, Y0 in lh.bands_of(BASE, (CAP, 2 * CAP)):                            # a rotation by 30 degrees cuts the corners: of the first
        assert outside[Y0:Y0 + BAND].mean() < 2 / 3, Y0                       # and the last rows at least a third (2365 pixels) is image
    band = lambda i, Y0: remap_ref.ref_remap(img[i:i + 1], fmap[Y0:Y0 + BAND], wr.BILINEAR, wr.CONSTANT, 173)[0]
    resampled(pkg, L, torch_cuda, rh.REMAP, img, (fmap, wr.BILINEAR, wr.CONSTANT, 173, 0), band, "remap")


def test_area_generic_kernel(pkg, L, torch_cuda):
    """blur_area_generic_kernel: 1400 x 1183 x 3 to the base shape, a reduction by no whole factor on either axis."""
    img = lh.own_ranges(np.random.default_rng(2206), lh.AREA_IN)
    h = img.shape[1]
    i_lo, i_hi, _, _ = area_ref.ref_axis(h, H)

    def band(i, Y0):
        lo, hi = int(i_lo[Y0]), int(i_hi[Y0 + BAND - 1]) + 1
        return area_ref.ref_area_rows(img[i:i + 1, lo:hi], lo, h, W, H, (Y0, Y0 + BAND))[0]
    resampled(pkg, L, torch_cuda, area_ref.AREA, img, (W, H), band, "area")


# ---------------------------------------------------------------- one thread per pixel: the colour transform
@pytest.mark.parametrize("case", [(lh.GREY9, 3, 1), (BASE, 1, 0), ((5, H, W, 3), 1, 0)], ids=["1to3-lut-9-images", "3to1-base", "3to1-5-images"])
def test_color_generic_kernel(pkg, L, torch_cuda, case):
    """blur_color_generic_kernel has one thread per PIXEL.  9 grey images of the base size to 3 channels with the LUT on are
    8 390 133 pixels: two trips and 1525 threads more, with the LUT that was put into LDS ahead of the loop.  3 -> 1 without
    a LUT is there for the channel stride: on the base shape, whose 2 796 711 pixels stay below the cap (two thirds of one
    trip), and on 5 such images, 4 661 185 pixels, which make one trip and a bit."""
    shape, co, lut_on = case
    n, h, w, c = shape
    rng = np.random.default_rng(2207 + co)
    img = lh.own_ranges(rng, shape)
    pixels = n * h * w
    assert (pixels > 2 * CAP) if co == 3 else (pixels < CAP) if n == 3 else (CAP < pixels < 2 * CAP)
    m, bias, shift, lut = color_ref.random_transform(rng, c, co, lut_on, 7, limit=False)
    k = make_color(pkg, m, bias, shift, lut)
    got = color_gpu_run(pkg, L, torch_cuda, img, k, offset_out=GUARD)
    assert rh.last(L) == color_ref.GENERIC == "blur_color_generic_kernel" and not color_ref.takes_tiled(shape)
    cpu = color_cpu_run(pkg, L, img, k, CPU_THREADS)
    units = [u for u in (CAP, 2 * CAP) if u < pixels]
    band = lambda i, r0: color_ref.ref_color(img[i:i + 1, r0:r0 + BAND], m, bias, shift, lut)[0]
    compare(got, cpu, lh.bands_of((n, h, w, co), units, co), band, case)
    assert len(np.unique(got)) > 100                                           # not saturated


# ---------------------------------------------------------------- tables, arithmetic, box, repack
def test_tables_generic_kernel(pkg, L, torch_cuda, base):
    """blur_tables_generic_kernel: a set of permutations per image and channel."""
    rng = np.random.default_rng(2209)
    img = np.array(base)
    tables = np.stack([np.stack([rng.permutation(256) for _ in range(CH)]) for _ in range(N)]).astype(np.uint8)
    got = lh.gpu_tables(pkg, L, torch_cuda, img, tables)
    assert rh.last(L) == hist_ref.TABLES_GENERIC == "blur_tables_generic_kernel"
    cpu = np.empty_like(img)
    pkg.check(L.mi_blur_cpu_run_tables(img.ctypes.data, cpu.ctypes.data, W, H, CH, N, tables.ctypes.data, CPU_THREADS), "mi_blur_cpu_run_tables")
    band = lambda i, r0: hist_ref.ref_apply(img[i:i + 1, r0:r0 + BAND], tables[i:i + 1])[0]
    compare(got, cpu, lh.bands_of(BASE, (CAP, 2 * CAP)), band, "tables")


@pytest.mark.parametrize("case", ["linear-shared-plane-b", "lerp-plane-mask"])
def test_arith_generic_kernel(pkg, L, torch_cuda, base, case):
    """blur_arith_generic_kernel: LINEAR with one plane B shared by the images (px = rem / channels and a stride of 0 on a
    later trip), and LERP with a full B and a plane mask per image (both strides)."""
    rng = np.random.default_rng(2210)
    a = np.array(base)
    if case == "linear-shared-plane-b":
        spec, b, m = arith_ref.lively_spec(rng, arith_ref.LINEAR), arith_ref.operand(rng, BASE, 1, 1), None
    else:
        spec, b, m = arith_ref.PRESETS["lerp"][1:], lh.own_ranges(rng, BASE)[::-1].copy(), arith_ref.operand(rng, BASE, 1, 0)
    k = arith_ref.struct_of(pkg, spec, b, m, BASE)
    assert (k.b_plane, k.b_shared, k.m_plane, k.m_shared) == ((1, 1, 0, 0) if m is None else (0, 0, 1, 0))
    assert not arith_ref.takes_flat(BASE, k) and not arith_ref.takes_plane(BASE, k)
    got = lh.gpu_arith(pkg, L, torch_cuda, k, a, b, m)
    assert rh.last(L) == arith_ref.GENERIC == "blur_arith_generic_kernel"
    cpu = lh.cpu_arith(pkg, L, k, a, b, m, CPU_THREADS)
    rows = lambda x, i, r0: None if x is None else x[(i if x.shape[0] > 1 else 0):(i if x.shape[0] > 1 else 0) + 1, r0:r0 + BAND]
    band = lambda i, r0: arith_ref.ref_arith(spec, rows(a, i, r0), rows(b, i, r0), rows(m, i, r0))[0]
    compare(got, cpu, lh.bands_of(BASE, (CAP, 2 * CAP)), band, case)
    assert len(np.unique(got)) > 100


@pytest.fixture(scope="module")
def base_tables(pkg, L, torch_cuda, base):
    """The base images and their two tables on the device, through blur_integral_generic_kernel and its cols kernel (rows of
    887 pixels: the 64-pixel carry runs 14 times); the tables themselves are checked in test_integral_generic_kernel."""
    d_in, ptr = lh.upload(torch_cuda, np.array(base))
    tabs = lh.device_tables(pkg, L, torch_cuda, ptr, BASE)
    yield d_in, ptr, tabs
    del d_in, tabs
    torch_cuda.cuda.empty_cache()


def test_integral_generic_kernel(pkg, L, base, base_tables):
    assert -(-W // 64) == 14
    S, Q = (lh.host_table(t, BASE) for t in base_tables[2])
    assert np.array_equal(S, box_ref.ref_integral(base)) and np.array_equal(Q, box_ref.ref_integral(base, True))


@pytest.mark.parametrize("radii", [(1, 1), (127, 127)], ids=lambda r: f"{r[0]}x{r[1]}")
@pytest.mark.parametrize("op", [box_ref.MEAN, box_ref.STDDEV, box_ref.THRESHOLD], ids=["mean", "stddev", "threshold"])
def test_box_generic_kernel(pkg, L, torch_cuda, base, base_tables, op, radii):
    """blur_box_generic_kernel from the device tables of the base shape."""
    d_in, ptr, tabs = base_tables
    img = np.array(base)
    rx, ry = radii
    k = lh.box_spec(pkg, op, rx, ry)
    got = lh.device_box(pkg, L, torch_cuda, ptr, tabs, BASE, k).cpu().numpy()
    assert rh.last(L) == box_ref.BOX_GENERIC == "blur_box_generic_kernel"
    cpu = lh.cpu_box(pkg, L, img, k, CPU_THREADS)

    def band(i, r0):
        lo, hi = max(r0 - ry, 0), min(r0 + BAND + ry, H)
        return box_ref.ref_box(img[i:i + 1, lo:hi], op, rx, ry, k.offset, k.invert)[0, r0 - lo:r0 - lo + BAND]
    compare(got, cpu, lh.bands_of(BASE, (CAP, 2 * CAP)), band, (op, radii))


@pytest.mark.parametrize("direction", ["planar_to_interleaved", "interleaved_to_planar"])
def test_repack_bytes_kernel(pkg, L, torch_cuda, base, direction):
    """repack_bytes_kernel<P2I>, both directions, against np.transpose.  The repack does not report its kernel; planes of
    932 237 pixels are no whole groups of 16, which is the rule of its other kernel (check_past_the_caps())."""
    torch = torch_cuda
    inter = np.array(base)
    planar = np.ascontiguousarray(inter.transpose(0, 3, 1, 2))
    src, want = (planar, inter) if direction == "planar_to_interleaved" else (inter, planar)
    d_src, p_src = lh.upload(torch, src)
    d_dst, p_dst = lh.guarded_bytes(torch, want.size)
    pkg.check(getattr(L, f"mi_blur_{direction}")(p_src, p_dst, W, H, CH, N, lh.stream(torch)), direction)
    torch.cuda.synchronize()
    assert lh.guards_intact(d_dst, want.size), "wrote outside the output"
    assert np.array_equal(d_dst[64:64 + want.size].cpu().numpy().reshape(want.shape), want)


# ---------------------------------------------------------------- the two other caps
@pytest.mark.parametrize("tables", ["s-and-q", "s", "q"])
def test_integral_generic_kernel_past_its_rows_cap(pkg, L, torch_cuda, tables):
    """blur_integral_generic_kernel on 9 x 29128 rows of 5 pixels: 262 152 rows, eight more than 65536 workgroups of 4 take
    in one trip, so the waves of the first two workgroups stride to the last eight rows of image 8.  (262 146 rows in 3
    images of 87382, two past the cap, are not to be had: the family takes at most 32768 rows an image, and 262 146 =
    2 * 3 * 43691 has no other factor below that.  That shape is refused up front, which is asserted.)"""
    shape = lh.ROWS_SHAPE
    assert shape[0] * shape[1] == ROW_CAP + 8
    img = lh.own_ranges(np.random.default_rng(2211), shape)
    want_s, want_q = tables != "q", tables != "s"
    d_in, ptr = lh.upload(torch_cuda, img)
    tabs = lh.device_tables(pkg, L, torch_cuda, ptr, shape, want_s, want_q)
    assert rh.last(L) == box_ref.INTEGRAL_GENERIC == "blur_integral_generic_kernel"
    cS, cQ = np.empty(shape, np.uint32), np.empty(shape, np.uint32)
    n, h, w, c = shape
    pkg.check(L.mi_blur_cpu_run_integral(img.ctypes.data, cS.ctypes.data, cQ.ctypes.data, w, h, c, n, CPU_THREADS), "mi_blur_cpu_run_integral")
    for t, cpu, square in zip(tabs, (cS, cQ), (False, True)):
        assert (t is not None) == (want_q if square else want_s)
        if t is not None:
            got = lh.host_table(t, shape)
            assert np.array_equal(got, cpu) and np.array_equal(got, box_ref.ref_integral(img, square)), square
    n, h, w, c = lh.ROWS_REFUSED
    p = [None if t is None else t.data_ptr() for t in tabs]
    assert L.mi_blur_enqueue_integral(ptr, p[0], p[1], w, h, c, n, ptr, lh.stream(torch_cuda)) == pkg.ERR_INVALID


def test_hist_generic_kernel_past_its_parts_cap(pkg, L, torch_cuda):
    """blur_hist_generic_kernel on one image of 1673 x 1673 x 3: 8 396 787 bytes are more than 256 workgroups x 32 768, so
    every workgroup strides.  Then the same image through mi_blur_enqueue_tone (EQUALIZE per channel): that histogram,
    blur_tone_table_kernel and blur_tables_generic_kernel past its own cap, three launches in a row."""
    torch = torch_cuda
    shape = lh.PARTS_SHAPE
    n, h, w, c = shape
    assert n * h * w * c > HIST_PARTS * HIST_PART_BYTES and n * h * w * c > 2 * CAP
    img = np.random.default_rng(2212).integers(0, 256, size=shape, dtype=np.uint8)
    img[0, :, :, 1] = (90 + img[0, :, :, 1] % 51).astype(np.uint8)                # a low-contrast channel: equalisation does something
    words = n * c * hist_ref.BINS
    d_in, ptr = lh.upload(torch, img)
    d_hist = torch.full((words + 32,), -1, dtype=torch.int32, device="cuda")
    pkg.check(L.mi_blur_enqueue_hist(ptr, d_hist.data_ptr(), w, h, c, n, lh.stream(torch)), "mi_blur_enqueue_hist")
    torch.cuda.synchronize()
    assert rh.last(L) == hist_ref.HIST_GENERIC == "blur_hist_generic_kernel"
    o = d_hist.cpu().numpy().view(np.uint32)
    assert (o[words:] == lh.ONES).all(), "wrote outside the histogram"
    want_hist = hist_ref.ref_hist(img)
    cpu_hist = np.empty((n, c, hist_ref.BINS), np.uint32)
    pkg.check(L.mi_blur_cpu_run_hist(img.ctypes.data, cpu_hist.ctypes.data, w, h, c, n, CPU_THREADS), "mi_blur_cpu_run_hist")
    assert np.array_equal(o[:words].reshape(n, c, hist_ref.BINS), want_hist) and np.array_equal(cpu_hist, want_hist)

    tone = pkg.Tone(hist_ref.EQUALIZE, 0, 0, 0, 0)
    want, _, want_tables = hist_ref.ref_tone(img, hist_ref.EQUALIZE)
    assert L.mi_blur_tone_work_bytes(c, n) == 5 * words
    d_work = torch.full((5 * words + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    d_out, p_out = lh.guarded_bytes(torch, img.size)
    pkg.check(L.mi_blur_enqueue_tone(ptr, p_out, w, h, c, n, C.byref(tone), d_work.data_ptr(), lh.stream(torch)), "mi_blur_enqueue_tone")
    torch.cuda.synchronize()
    assert rh.last(L) == hist_ref.TABLES_GENERIC == "blur_tables_generic_kernel"
    wk = d_work.cpu().numpy()
    assert lh.guards_intact(d_out, img.size) and (wk[5 * words:] == 0x5A).all()
    assert np.array_equal(wk[:4 * words].view(np.uint32).reshape(n, c, hist_ref.BINS), want_hist)
    assert np.array_equal(wk[4 * words:5 * words].reshape(n, c, hist_ref.BINS), want_tables)
    got = d_out[64:64 + img.size].cpu().numpy().reshape(shape)
    cpu_out = np.empty_like(img)
    pkg.check(L.mi_blur_cpu_run_tone(img.ctypes.data, cpu_out.ctypes.data, w, h, c, n, C.byref(tone), None, CPU_THREADS), "mi_blur_cpu_run_tone")
    assert np.array_equal(got, want) and np.array_equal(cpu_out, want)
    assert not np.array_equal(want_tables[0, 1], np.arange(256))
