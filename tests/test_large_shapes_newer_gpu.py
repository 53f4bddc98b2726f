"""Large and extreme shapes on a real MI355X (-m gpu) for the families that came after tests/test_large_shapes_gpu.py: the
two-image arithmetic, the integral images with the box filters made from them, the area resize and the remap.  One-row,
one-column, very wide and very tall frames, area and remap at MI_BLUR_RESIZE_MAX_DIM, one image within 75 kB of 2^31
bytes and batches beyond it.  What is under test is the offset arithmetic: row times pitch kept in 32 bits in the area kernel,
table offsets of 2^31 words and 2^33 bytes and thousands of bands handed from dispatch to dispatch in the integral, image
times stride with a shared plane in the arithmetic, Q11 map entries of 2^25 and more in the remap.  Byte for byte (word
for word) against the numpy restatements, on bands of 8 rows where the image is too large to restate whole.

The arithmetic, the integral and the box filters take at most MI_BLUR_RESIZE_MAX_DIM = 32768 pixels a side (the histogram
family's limits, include/mi_blur.h), so every shape of EXTREME below, and an image of 65535 rows, is refused by them up
front: that is asserted, for every entry point, and the launches run on ADMITTED, the same shapes cut to that limit."""
import ctypes as C

import numpy as np
import pytest

import area_ref
import arith_ref
import box_ref
import large_harness as lh
import remap_ref
import resample_harness as rh
import warp_ref as wr
from area_ref import AREA
from filter_harness import torch_cuda  # noqa: F401
from large_harness import BAND
from resize_ref import MAX_DIM

pytestmark = pytest.mark.gpu

# restated from tests/test_large_shapes_gpu.py
EXTREME = [(1, 100000, 3), (100000, 1, 3), (3, 65536, 4), (70000, 16, 1), (2, 1000003, 1), (65537, 48, 2)]
BIG_H, BIG_W, BIG_C = 26757, 26752, 3          # 80256-byte rows: whole 32-byte pairs and whole groups of six chunks
assert BIG_W * BIG_H * BIG_C < 2 ** 31 <= BIG_W * (BIG_H + 1) * BIG_C
# EXTREME within the limit: one row; one column; 8192 chunks per row; one chunk per row and 2048 bands of the integral; a
# ragged row; 6 chunks per row and the most rows an image may have
ADMITTED = [(1, MAX_DIM, 3), (MAX_DIM, 1, 3), (3, MAX_DIM, 4), (MAX_DIM, 16, 1), (2, MAX_DIM - 1, 1), (MAX_DIM, 48, 2)]
assert all(max(h, w) > MAX_DIM for h, w, c in EXTREME) and [c for _, _, c in ADMITTED] == [c for _, _, c in EXTREME]
OPS = (box_ref.MEAN, box_ref.STDDEV, box_ref.THRESHOLD)
LERP, ABSDIFF = arith_ref.PRESETS["lerp"][1:], arith_ref.PRESETS["absdiff"][1:]


def shape_id(s):
    return "x".join(map(str, s))


def band_starts(h):
    """First rows of the compared bands: the top, around the 2^30-byte offset (13380 rows of 80256 bytes are just past
    it), the middle, the bottom."""
    return (0, min(13376, h - BAND), h // 2 + 5, h - BAND)


def big_random(torch, h, seed=11, w=BIG_W, c=BIG_C):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(0, 256, (h, w, c), dtype=torch.uint8, device="cuda", generator=g)


def slab(d_in, lo, hi):
    return np.ascontiguousarray(d_in[lo:hi].cpu().numpy())[None]


# ---------------------------------------------------------------- extreme aspect ratios
@pytest.mark.parametrize("shape", EXTREME, ids=shape_id)
def test_beyond_the_limit_is_refused_up_front(pkg, L, torch_cuda, shape):
    """More than 32768 pixels a side: MI_BLUR_ERR_INVALID from every entry point of the three families, before any launch
    (the buffers are 64 bytes and stay untouched)."""
    h, w, c = shape
    d = torch_cuda.zeros(4 * 64, dtype=torch_cuda.uint8, device="cuda")
    a, b, m, o = (d.data_ptr() + 64 * i for i in range(4))
    s = lh.stream(torch_cuda)
    for k, mask in ((pkg.arith_preset("absdiff"), None), (pkg.arith_preset("lerp"), m)):
        assert L.mi_blur_enqueue_arith(a, b, mask, o, w, h, c, 1, C.byref(k), s) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_integral(a, b, m, w, h, c, 1, o, s) == pkg.ERR_INVALID
    for op in OPS:
        k = lh.box_spec(pkg, op, 1, 1)
        assert L.mi_blur_enqueue_box_from_integral(a if op == box_ref.THRESHOLD else None, b, m if op == box_ref.STDDEV else None, o, w, h, c, 1, C.byref(k), s) == pkg.ERR_INVALID
        assert L.mi_blur_enqueue_box(a, o, w, h, c, 1, C.byref(k), b, s) == pkg.ERR_INVALID
    torch_cuda.cuda.synchronize()
    assert not bool(d.any())


@pytest.mark.parametrize("shape", ADMITTED, ids=shape_id)
def test_extreme_aspect_ratios_arith(pkg, L, torch_cuda, shape):
    """ABSDIFF of two full operands and LERP through a plane mask, in the kernel arith_ref's rules name."""
    rng = np.random.default_rng(sum(shape))
    full = (1,) + shape
    a, b = (rng.integers(0, 256, size=full, dtype=np.uint8) for _ in range(2))
    m = arith_ref.operand(rng, full, 1, 0)
    ragged = shape[0] * shape[1] % 16 != 0
    assert ragged == (shape == (2, MAX_DIM - 1, 1))
    for spec, mask in ((ABSDIFF, None), (LERP, m)):
        k = arith_ref.struct_of(pkg, spec, b, mask, full)
        kernel = arith_ref.FLAT if arith_ref.takes_flat(full, k) else arith_ref.PLANE if arith_ref.takes_plane(full, k) else arith_ref.GENERIC
        # the ragged row is generic; a plane mask of a one-channel image is a full operand
        assert kernel == (arith_ref.GENERIC if ragged else arith_ref.PLANE if mask is not None and shape[2] > 1 else arith_ref.FLAT)
        got = lh.gpu_arith(pkg, L, torch_cuda, k, a, b, mask)
        assert rh.last(L) == kernel, (shape, spec)
        assert np.array_equal(got, arith_ref.ref_arith(spec, a, b, mask)), (shape, spec)


@pytest.mark.parametrize("radii", [(1, 1), (127, 127)], ids=lambda r: f"r{r[0]}")
@pytest.mark.parametrize("shape", ADMITTED + [(3, 8192, 4)], ids=shape_id)
def test_extreme_aspect_ratios_integral_and_box(pkg, L, torch_cuda, shape, radii):
    """S and Q in one launch against ref_integral, then MEAN, STDDEV and THRESHOLD from those tables at (1, 1) or at
    (127, 127) against ref_box: on the one-row and the one-column image every window clamps on both sides at once.
    32768 x 16 x 1 is the tiled integral with one wave and 2048 bands, 32768 x 48 x 2 and 3 x 8192 x 4 (the widest tiled
    row) are tiled too, the others generic.  (One case per radius: ref_box of STDDEV on the whole image is what takes the
    time here, not the launches.)"""
    torch = torch_cuda
    full = (1,) + shape
    h, w, c = shape
    img = np.random.default_rng(sum(shape)).integers(0, 256, size=full, dtype=np.uint8)
    assert box_ref.integral_takes_tiled(full) == (shape in ((MAX_DIM, 16, 1), (MAX_DIM, 48, 2), (3, 8192, 4)))
    d_in, ptr = lh.upload(torch, img)
    tabs = lh.device_tables(pkg, L, torch, ptr, full)                               # asserts the kernel from the rule
    assert np.array_equal(lh.host_table(tabs[0], full), box_ref.ref_integral(img)), shape
    assert np.array_equal(lh.host_table(tabs[1], full), box_ref.ref_integral(img, True)), shape
    rx, ry = radii
    for op in OPS:
        k = lh.box_spec(pkg, op, rx, ry)
        got = lh.device_box(pkg, L, torch, ptr, tabs, full, k).cpu().numpy()
        assert rh.last(L) == (box_ref.BOX_TILED if box_ref.box_takes_tiled(full) else box_ref.BOX_GENERIC), (shape, op)
        assert np.array_equal(got, box_ref.ref_box(img, op, rx, ry, k.offset, k.invert)), (shape, op, rx, ry)


# (input h, w, c), Wo, Ho: the 64x cap on a full-width row; on a full-height column; equal width and many strips; no whole
# ratio; a one-column image
AREA_EXTREME = [((2, MAX_DIM, 1), 512, 1), ((MAX_DIM, 16, 1), 16, 512), ((3, MAX_DIM, 4), MAX_DIM, 3), ((2, MAX_DIM, 1), 12345, 1), ((16, 1, 3), 1, 7)]


@pytest.mark.parametrize("case", AREA_EXTREME, ids=lambda c: shape_id(c[0]) + f"-{c[1]}x{c[2]}")
def test_extreme_aspect_ratios_area(pkg, L, torch_cuda, case):
    """To and from MI_BLUR_RESIZE_MAX_DIM, against the prefix-sum restatement (a weight matrix of 32768 x 32768 would not
    fit); one past the limit on either side of either size is refused before any launch."""
    shape, wo, ho = case
    h, w, c = shape
    full = (1,) + shape
    img = np.random.default_rng(wo + ho).integers(0, 256, size=full, dtype=np.uint8)
    assert area_ref.valid(full, wo, ho)
    got = rh.gpu_run(AREA, pkg, L, torch_cuda, img, (wo, ho), offset_out=64)
    assert rh.last(L) == (AREA.tiled if area_ref.takes_tiled(full, wo, ho, 0, 64) else AREA.generic), case
    assert np.array_equal(got, area_ref.ref_area_rows(img, 0, h, wo, ho, (0, ho))), case
    if wo == w and ho == h:
        assert np.array_equal(got, img)
    d = torch_cuda.zeros(64, dtype=torch_cuda.uint8, device="cuda")                   # never touched
    for (wi, hi), (wo2, ho2) in (((MAX_DIM + 1, h), (wo, ho)), ((w, MAX_DIM + 1), (wo, ho)), ((w, h), (MAX_DIM + 1, ho)), ((w, h), (wo, MAX_DIM + 1))):
        r = pkg.Area(wo2, ho2)
        assert L.mi_blur_enqueue_area(d.data_ptr(), d.data_ptr() + 32, wi, hi, c, 1, C.byref(r), None) == pkg.ERR_INVALID
    assert not bool(d.any())


def scaled_identity(w, h, wo, ho):
    """Output (X, Y) reads the position (X W / Wo, Y H / Ho), floored to 1/2048 pixel."""
    m = remap_ref.identity_map(wo, ho).astype(np.int64)
    m[:, :, 0] = m[:, :, 0] * w // wo
    m[:, :, 1] = m[:, :, 1] * h // ho
    return m.astype(np.int32)


# (input h, w, c), (Wo, Ho)
REMAP_EXTREME = [((33, 48, 3), (MAX_DIM, 1)), ((33, 48, 3), (1, MAX_DIM)), ((33, 48, 3), (16, MAX_DIM)), ((1, MAX_DIM, 1), (64, 32)), ((MAX_DIM, 16, 1), (64, 32))]


@pytest.mark.parametrize("border", [wr.CLAMP, wr.CONSTANT], ids=["clamp", "constant"])
@pytest.mark.parametrize("case", REMAP_EXTREME, ids=lambda c: shape_id(c[0]) + f"-{c[1][0]}x{c[1][1]}")
def test_extreme_aspect_ratios_remap(pkg, L, torch_cuda, case, border):
    """32768 pixels along one axis of the output or of the input, under the identity scaled to the output and under the
    map with the extreme entries: BILINEAR in the kernel the rule names (the tiled one, but for the output of one column),
    NEAREST and an output 7 bytes off alignment in the generic one."""
    shape, (wo, ho) = case
    h, w, c = shape
    full = (1,) + shape
    img = wr.edge_image(np.random.default_rng(sum(shape) + wo), *full)
    assert max(h, w, wo, ho) == MAX_DIM
    assert remap_ref.takes_tiled(full, wo, ho, wr.BILINEAR, 0, 64) == (wo != 1)
    for fmap in (scaled_identity(w, h, wo, ho), remap_ref.extremes_map(w, h, wo, ho)):
        for mode, offset_out in ((wr.BILINEAR, 64), (wr.NEAREST, 64), (wr.BILINEAR, 7)):
            got = rh.gpu_run(rh.REMAP, pkg, L, torch_cuda, img, (fmap, mode, border, 173, 0), offset_out=offset_out)
            assert rh.last(L) == rh.REMAP.kernel(full, (fmap, mode, border, 173, 0), 0, offset_out), (mode, offset_out)
            assert offset_out == 64 and mode == wr.BILINEAR or rh.last(L) == rh.REMAP.generic
            assert np.array_equal(got, remap_ref.ref_remap(img, fmap, mode, border, 173)), (mode, offset_out)


# ---------------------------------------------------------------- one image near 2^31 bytes, and batches beyond
def enqueue_arith(pkg, L, torch, k, a, b, m, out, w, h, c, n):
    return L.mi_blur_enqueue_arith(a.data_ptr(), b.data_ptr(), None if m is None else m.data_ptr(), out, w, h, c, n, C.byref(k), lh.stream(torch))


def test_single_image_near_the_2gib_limit_arith_flat(pkg, L, torch_cuda):
    """A, B, the mask and the output of 26757 x 26752 x 3 each, ABSDIFF and LERP through the flat kernel; bands against
    numpy; one more row is refused."""
    torch = torch_cuda
    size = BIG_H * BIG_W * BIG_C
    d_a, d_b, d_m = (big_random(torch, BIG_H, seed) for seed in (11, 12, 13))
    d_out, p_out = lh.guarded_bytes(torch, size)
    try:
        for spec, mask in ((ABSDIFF, None), (LERP, d_m)):
            k = pkg.Arith(*spec)
            assert arith_ref.takes_flat((1, BIG_H, BIG_W, BIG_C), k)
            d_out.fill_(0x5A)
            pkg.check(enqueue_arith(pkg, L, torch, k, d_a, d_b, mask, p_out, BIG_W, BIG_H, BIG_C, 1), "mi_blur_enqueue_arith")
            torch.cuda.synchronize()
            assert rh.last(L) == arith_ref.FLAT and lh.guards_intact(d_out, size), "wrote outside the output"
            got = d_out[64:64 + size].view(BIG_H, BIG_W, BIG_C)
            for r0 in band_starts(BIG_H):
                rows = [None if t is None else slab(t, r0, r0 + BAND) for t in (d_a, d_b, mask)]
                assert np.array_equal(got[r0:r0 + BAND].cpu().numpy(), arith_ref.ref_arith(spec, *rows)[0]), (spec, r0)
            assert enqueue_arith(pkg, L, torch, k, d_a, d_b, mask, p_out, BIG_W, BIG_H + 1, BIG_C, 1) == pkg.ERR_INVALID
    finally:
        del d_a, d_b, d_m, d_out
        torch.cuda.empty_cache()


def test_batch_beyond_2gib_arith_plane_with_a_shared_plane(pkg, L, torch_cuda):
    """3 images of 16384 x 16384 x 4, 3 GiB, so the third image starts beyond 2^31, and ONE one-channel plane B for all of
    them: img * b_stride must be 0 for it and 64 bits wide for A and the output.  Filled on the device with the tiled
    4096-byte pattern of tests/test_color_gpu.py plus the image index; the first and the last 4 rows of every image."""
    torch = torch_cuda
    n, h, w, c = 3, 16384, 16384, 4
    isz = h * w * c
    pattern = ((np.arange(4096, dtype=np.int64) * 37 + (np.arange(4096) >> 5) * 11) % 251).astype(np.uint8)
    plane = ((np.arange(4096, dtype=np.int64) * 53 + (np.arange(4096) >> 4) * 7) % 256).astype(np.uint8)
    d_a = torch.empty(n * isz, dtype=torch.uint8, device="cuda")
    d_b = torch.empty(h * w, dtype=torch.uint8, device="cuda")
    d_out, p_out = lh.guarded_bytes(torch, n * isz)
    try:
        d_pat = torch.from_numpy(pattern).cuda()
        for i in range(n):
            d_a[i * isz:(i + 1) * isz].view(-1, 4096)[:] = d_pat + i
        d_b.view(-1, 4096)[:] = torch.from_numpy(plane).cuda()
        spec = (arith_ref.LINEAR, 3, -2, 40, 1)
        k = pkg.Arith(*spec, 1, 1, 0, 0)
        assert arith_ref.takes_plane((n, h, w, c), k)
        pkg.check(enqueue_arith(pkg, L, torch, k, d_a, d_b, None, p_out, w, h, c, n), "mi_blur_enqueue_arith")
        torch.cuda.synchronize()
        assert rh.last(L) == arith_ref.PLANE and lh.guards_intact(d_out, n * isz), "wrote outside the output"
        rows = 4
        b4 = np.tile(plane, rows * w // 4096).reshape(1, rows, w, 1)
        for i in range(n):
            a4 = (np.tile(pattern, rows * w * c // 4096) + np.uint8(i)).reshape(1, rows, w, c)
            want = arith_ref.ref_arith(spec, a4, b4)
            assert len(np.unique(want)) > 50
            for first in (0, isz - rows * w * c):
                got = d_out[64 + i * isz + first:64 + i * isz + first + rows * w * c].cpu().numpy()
                assert np.array_equal(got, want.reshape(-1)), (i, first)
    finally:
        del d_a, d_b, d_out
        torch.cuda.empty_cache()


def check_table_bands(torch, d_img, table, starts, square):
    """Rows of one image's table (int32 device tensor H x W x C) against torch_integral_rows(), on the device."""
    want = box_ref.torch_integral_rows(torch, d_img, starts, BAND, square, chunk=1024)
    for r in starts:
        got = table[r:r + BAND].to(torch.int64) & 0xFFFFFFFF
        assert bool((got == want[r]).all()), (square, r)
    del want


def test_two_images_of_the_tallest_tiled_integral_and_their_box_filters(pkg, L, torch_cuda):
    """2 images of 32768 x 8192 x 4, the tallest and widest the tiled integral takes (an image of 65535 rows, one row short
    of 2^31 bytes, is over the family's limit of 32768 rows and is refused): 2 GiB in, S and Q of 8.6 GB each in one
    launch, a work buffer of 1.07 GB for 2 x 2048 bands.  The tables' word offsets reach 2^31 and their byte offsets 2^33;
    first = (img * H + y0) * row_e runs with img = 1.  Bands of both images against column sums of all rows above, taken in
    torch in chunks, then a cumulative sum along the row, modulo 2^32; then all three box filters from those tables at
    (1, 1) and (127, 15), against ref_box of the slab with ry halo rows: on the same bands of image 1, and on the first and
    the last band of image 0 (fewer bands than the tables, for the suite's time: profiles/r22_large_shapes.md)."""
    torch = torch_cuda
    n, h, w, c = 2, MAX_DIM, 8192, 4
    shape = (n, h, w, c)
    assert box_ref.integral_takes_tiled(shape) and n * h * w * c == 2 ** 31
    g = torch.Generator(device="cuda")
    g.manual_seed(21)
    d_in = torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
    tabs = None
    try:
        tabs = lh.device_tables(pkg, L, torch, d_in.data_ptr(), shape)              # asserts blur_integral_tiled_kernel and the guards
        starts = band_starts(h)
        for i in range(n):
            for t, square in zip(tabs, (False, True)):
                check_table_bands(torch, d_in[i], t.view(shape)[i], starts, square)
        for rx, ry in ((1, 1), (127, 15)):
            for op in OPS:
                k = lh.box_spec(pkg, op, rx, ry)
                d_out = lh.device_box(pkg, L, torch, d_in.data_ptr(), tabs, shape, k)
                assert rh.last(L) == box_ref.BOX_TILED
                for i in range(n):
                    for r0 in (starts if i == n - 1 else (starts[0], starts[-1])):    # image 0: its first and last band only
                        lo, hi = max(r0 - ry, 0), min(r0 + BAND + ry, h)
                        want = box_ref.ref_box(slab(d_in[i], lo, hi), op, rx, ry, k.offset, k.invert)[0, r0 - lo:r0 - lo + BAND]
                        assert np.array_equal(d_out[i, r0:r0 + BAND].cpu().numpy(), want), (op, rx, ry, i, r0)
                del d_out
        d = torch.zeros(64, dtype=torch.uint8, device="cuda")
        for rows in (MAX_DIM + 1, 65535):
            assert L.mi_blur_enqueue_integral(d_in.data_ptr(), tabs[0].data_ptr(), tabs[1].data_ptr(), w, rows, c, 1, d.data_ptr(), None) == pkg.ERR_INVALID
    finally:
        del d_in, tabs
        torch.cuda.empty_cache()


def test_single_image_near_the_2gib_limit_integral_generic(pkg, L, torch_cuda):
    """26757 x 26752 x 3 is generic because W > 8192: S alone, 8.6 GB, the same row reference; one more row is refused."""
    torch = torch_cuda
    shape = (1, BIG_H, BIG_W, BIG_C)
    assert not box_ref.integral_takes_tiled(shape)
    d_in = big_random(torch, BIG_H)
    tabs = None
    try:
        tabs = lh.device_tables(pkg, L, torch, d_in.data_ptr(), shape, True, False)  # asserts blur_integral_generic_kernel and the guards
        check_table_bands(torch, d_in, tabs[0].view(shape)[0], band_starts(BIG_H), False)
        d = torch.zeros(64, dtype=torch.uint8, device="cuda")
        assert L.mi_blur_enqueue_integral(d_in.data_ptr(), tabs[0].data_ptr(), None, BIG_W, BIG_H + 1, BIG_C, 1, d.data_ptr(), None) == pkg.ERR_INVALID
        k = lh.box_spec(pkg, box_ref.MEAN, 1, 1)                                   # ... by the box filters too, from tables and fused
        assert L.mi_blur_enqueue_box_from_integral(None, tabs[0].data_ptr(), None, d_in.data_ptr(), BIG_W, BIG_H + 1, BIG_C, 1, C.byref(k), None) == pkg.ERR_INVALID
        assert L.mi_blur_enqueue_box(d_in.data_ptr(), tabs[0].data_ptr(), BIG_W, BIG_H + 1, BIG_C, 1, C.byref(k), d.data_ptr(), None) == pkg.ERR_INVALID
    finally:
        del d_in, tabs
        torch.cuda.empty_cache()


def test_single_image_near_the_2gib_limit_area(pkg, L, torch_cuda):
    """26757 x 26752 x 3 to 13360 x 13379: no whole ratio on either axis, both images eligible for the tiled kernel, whose
    (unsigned) row * pitch products come within 75 kB of 2^31 on the input.  Bands against the prefix-sum restatement of the
    slab of input rows i_lo(Y0) .. i_hi(Y0 + 7); one more input row is refused."""
    torch = torch_cuda
    wo, ho = 13360, 13379
    assert area_ref.takes_tiled((1, BIG_H, BIG_W, BIG_C), wo, ho) and BIG_H % ho and BIG_W % wo
    i_lo, i_hi, _, _ = area_ref.ref_axis(BIG_H, ho)
    d_in = big_random(torch, BIG_H)
    size = ho * wo * BIG_C
    d_out, p_out = lh.guarded_bytes(torch, size)
    try:
        r = pkg.Area(wo, ho)
        pkg.check(L.mi_blur_enqueue_area(d_in.data_ptr(), p_out, BIG_W, BIG_H, BIG_C, 1, C.byref(r), None), "mi_blur_enqueue_area")
        torch.cuda.synchronize()
        assert rh.last(L) == AREA.tiled and lh.guards_intact(d_out, size), "wrote outside the output"
        got = d_out[64:64 + size].view(ho, wo, BIG_C)
        for Y0 in band_starts(ho):
            lo, hi = int(i_lo[Y0]), int(i_hi[Y0 + BAND - 1]) + 1
            want = area_ref.ref_area_rows(slab(d_in, lo, hi), lo, BIG_H, wo, ho, (Y0, Y0 + BAND))[0]
            assert np.array_equal(got[Y0:Y0 + BAND].cpu().numpy(), want), Y0
        assert L.mi_blur_enqueue_area(d_in.data_ptr(), p_out, BIG_W, BIG_H + 1, BIG_C, 1, C.byref(r), None) == pkg.ERR_INVALID
    finally:
        del d_in, d_out
        torch.cuda.empty_cache()


def test_single_image_near_the_2gib_limit_remap(pkg, L, torch_cuda):
    """The INPUT near 2^31 bytes: 64 output rows of 26752 pixels read from its first rows, from the rows around the
    2^30-byte offset and from its last rows and beyond them (map entries of 26757 * 2048 > 2^25), under both borders:
    BILINEAR through the tiled kernel, NEAREST through the generic one.  Bands against ref_remap_slab on the rows the
    band's map reads."""
    torch = torch_cuda
    ho, wo = 64, BIG_W
    size = ho * wo * BIG_C
    d_in = big_random(torch, BIG_H)
    d_out, p_out = lh.guarded_bytes(torch, size)
    try:
        for first_row in (0, 13376, BIG_H - 60):                                   # the last: output rows 60.. read past the last input row
            fmap = remap_ref.affine_map([wr.Q, 0, 3 * wr.Q // 8 + 1, 0, wr.Q, first_row * wr.Q + 5 * wr.Q // 8], wo, ho)
            assert fmap[:, :, 1].max() >= (first_row + ho - 1) * remap_ref.ONE
            d_map = torch.from_numpy(fmap).cuda()
            assert d_map.data_ptr() % 16 == 0
            for mode, kernel in ((wr.BILINEAR, rh.REMAP.tiled), (wr.NEAREST, rh.REMAP.generic)):
                assert remap_ref.takes_tiled((1, BIG_H, BIG_W, BIG_C), wo, ho, mode) == (mode == wr.BILINEAR)
                for border in (wr.CLAMP, wr.CONSTANT):
                    d_out.fill_(0x5A)
                    rm = remap_ref.make_remap(pkg, wo, ho, mode, border, 173)
                    pkg.check(L.mi_blur_enqueue_remap(d_in.data_ptr(), p_out, BIG_W, BIG_H, BIG_C, 1, C.byref(rm), d_map.data_ptr(), lh.stream(torch)), "mi_blur_enqueue_remap")
                    torch.cuda.synchronize()
                    assert rh.last(L) == kernel, (mode, first_row, border)
                    assert lh.guards_intact(d_out, size), "wrote outside the output"
                    got = d_out[64:64 + size].view(ho, wo, BIG_C)
                    for Y0 in (0, 28, ho - BAND):                                  # 28: across the two tile rows
                        band = fmap[Y0:Y0 + BAND]
                        lo, hi = remap_ref.map_rows(band, mode, BIG_W, BIG_H)
                        want = remap_ref.ref_remap_slab(slab(d_in, lo, hi + 1), lo, BIG_H, band, mode, border, 173)[0]
                        assert np.array_equal(got[Y0:Y0 + BAND].cpu().numpy(), want), (mode, first_row, border, Y0)
            del d_map
        last = fmap[ho - BAND:]                                                    # the last band of the last map runs off the bottom, not wholly
        assert last[:, :, 1].max() > BIG_H * remap_ref.ONE > last[:, :, 1].min()
        rm = remap_ref.make_remap(pkg, wo, ho, wr.BILINEAR, wr.CONSTANT, 173)
        d_map = torch.from_numpy(fmap).cuda()
        assert L.mi_blur_enqueue_remap(d_in.data_ptr(), p_out, BIG_W, BIG_H + 1, BIG_C, 1, C.byref(rm), d_map.data_ptr(), None) == pkg.ERR_INVALID
    finally:
        del d_in, d_out
        torch.cuda.empty_cache()
