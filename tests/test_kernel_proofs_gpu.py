"""Kernel proofs and geometry sweeps on a real MI355X (-m gpu), against references computed from the definitions in
include/mi_blur.h (kernel_proofs.py), never from the product; every launch also asserts which kernel ran.

  * blur_median_fast_kernel, all 8 instantiations: exhaustive by the 0-1 principle (kernel_proofs.py).  The interior
    stream puts every two-valued window on every interior row at every byte position its channel can take in a chunk;
    the edge batch enumerates the first and last 2r columns.
  * blur_median_generic_kernel: two-valued images of every adjacent pair (v, v+1) and every (0, v), window counts on K
    and K+1, radius 1..7.
  * blur_sep_tiled_kernel and blur_median_fast_kernel: chunk counts, rows, radius buckets, bands and grids at and next
    to the tile / wave boundaries; one-hot taps at every offset of every radius bucket.
  * blur_morph_tiled_kernel: proved window by window.  min / max compose to the min / max over a set of source
    positions, so the kernel is right iff that set is right; the proof images (morph_ref.py) hold isolated impulses that
    witness every (byte position, offset) pair at every radius (test_kernel_proofs_host.py checks that they do).
  * blur_morph_tiled_kernel, blur_bilateral_tiled_kernel, blur_conv_tiled_kernel: the sep kernel's geometry sweep, bands
    and grids, each filter walking its own kernel's bucket edges; blur_sep_down_tiled_kernel and blur_resize_tiled_kernel:
    chunk and row counts around their tiles, every phase, the sizes around 1x, 2x and 3x; blur_warp_tiled_kernel: output
    widths around its 64-pixel strips and heights around its tile rows, under translations, a rotation, an enlargement, a
    reduction and a map that leaves the image, both borders."""
import math

import numpy as np
import pytest

import conv_ref as cr
import kernel_proofs as kp
import morph_ref as mr
from filter_harness import (BILATERAL, CONV, MORPH, SEP, check_bands_and_grids, check_tiled_geometry_sweep, dev_run, random_bytes,  # noqa: F401
                            torch_cuda)
import resample_harness as rh
from resize_ref import BILINEAR, ref_resize, takes_tiled
import warp_ref as wr

pytestmark = pytest.mark.gpu

FAST, GENERIC = b"blur_median_fast_kernel", b"blur_median_generic_kernel"
TILED = b"blur_sep_tiled_kernel"
GUARD = 256


# ---------------------------------------------------------------- launches on device tensors, guard bytes around the output
def median_dev(pkg, L, torch, d_img, r, y0=None, y1=None, offset_in=0):
    """d_img (N, H, W, C) uint8 on the device -> the median through mi_blur_enqueue_median (_band for y0 / y1)."""
    n, h, w, c = d_img.shape
    y0 = 0 if y0 is None else y0
    y1 = h if y1 is None else y1
    if offset_in:
        buf = torch.zeros(d_img.numel() + 64, dtype=torch.uint8, device="cuda")
        buf[offset_in:offset_in + d_img.numel()] = d_img.reshape(-1)
        src = buf.data_ptr() + offset_in
    else:
        src = d_img.data_ptr()
    size = n * (y1 - y0) * w * c
    out = torch.full((size + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if y0 == 0 and y1 == h:
        rc = L.mi_blur_enqueue_median(src, out.data_ptr() + GUARD, w, h, c, r, n, s)
    else:
        assert n == 1
        rc = L.mi_blur_enqueue_median_band(src, out.data_ptr() + GUARD, w, h, c, r, y0, y1, s)
    pkg.check(rc, "mi_blur_enqueue_median")
    torch.cuda.synchronize()
    assert bool((out[:GUARD] == 0x5A).all()) and bool((out[GUARD + size:] == 0x5A).all()), "wrote outside the output"
    return out[GUARD:GUARD + size].reshape(n, y1 - y0, w, c)


def sep_dev(pkg, L, torch, d_img, wx, wy, y0=None, y1=None):
    return dev_run(SEP, pkg, L, torch, d_img, pkg.SepKernel.from_taps(wx, wy), y0, y1)


def assert_same(torch, got, want, what):
    bad = got != want
    nbad = int(bad.sum())
    if nbad:
        first = torch.nonzero(bad)[0].tolist()
        pytest.fail(f"{what}: {nbad} outputs differ, first at (n, y, x, c) = {first}: got {int(got[tuple(first)])}, "
                    f"want {int(want[tuple(first)])}")


# ---------------------------------------------------------------- the median proof (0-1 principle)
def high_count_dev(torch, mask, r):
    """torch form of kernel_proofs.high_count_np: high values in the clamped window of every pixel."""
    n, h, w, c = mask.shape
    v = torch.zeros_like(mask)
    for j in range(-r, r + 1):
        v += mask[:, [min(max(y + j, 0), h - 1) for y in range(h)]]
    p = torch.cat([v[:, :, :1].expand(n, h, r, c), v, v[:, :, -1:].expand(n, h, r, c)], dim=2)
    del v
    cnt = torch.zeros_like(mask)
    for i in range(2 * r + 1):
        cnt += p[:, :, i:i + w]
    return cnt


def stream_mask_dev(torch, seq_d, r, c, shift):
    """torch form of kernel_proofs.stream_mask_np, built on the device."""
    d, n = 2 * r + 1, seq_d.numel()
    h, w = kp.med_bh(r) + 2 * r, kp.stream_width(r, c, shift)
    mask = torch.empty((1, h, w, c), dtype=torch.uint8, device="cuda")
    x = torch.arange(w, dtype=torch.int64, device="cuda")
    for ch in range(c):
        v = seq_d[(x + (n - shift) + ch * kp.CHANNEL_OFFSET) % n]
        for y in range(h):
            mask[0, y, :, ch] = ((v >> kp.row_bit(y, ch, d)) & 1) ^ (ch & 1)
        del v
    return mask


def check_two_valued(pkg, L, torch, mask, r, what):
    cnt = high_count_dev(torch, mask, r)
    k = ((2 * r + 1) ** 2 - 1) // 2
    above = cnt >= k + 1
    del cnt
    for lo, hi in kp.MEDIAN_PAIRS:
        img = mask * (hi - lo)                           # uint8 throughout: the pattern sets reach a gigabyte
        img += lo
        got = median_dev(pkg, L, torch, img, r)
        assert L.mi_blur_last_kernel() == FAST, what
        del img
        want = above.to(torch.uint8) * (hi - lo)
        want += lo
        assert_same(torch, got, want, f"{what}, values ({lo}, {hi})")
        del got, want


@pytest.mark.parametrize("r", [1, 2])
def test_median_fast_proof_interior(pkg, L, torch_cuda, r):
    """Every two-valued window on every interior row (every phase of the lane's row band), at every byte position of
    every channel in a 16-byte chunk (one launch per pad shift), for both value pairs and 1..4 channels."""
    torch = torch_cuda
    d = 2 * r + 1
    seq_d = torch.from_numpy(kp.debruijn(d, d)).cuda()
    for c in range(1, 5):
        for shift in range(16 // math.gcd(c, 16)):
            mask = stream_mask_dev(torch, seq_d, r, c, shift)
            assert mask.numel() <= 2 ** 31 - 1
            check_two_valued(pkg, L, torch, mask, r, f"r={r} C={c} shift={shift}")
            del mask
            torch.cuda.empty_cache()


@pytest.mark.parametrize("r", [1, 2])
def test_median_fast_proof_edges(pkg, L, torch_cuda, r):
    """Every combination of the first 2r and, independently, of the last 2r column values: x = 0 .. 2r-1 and the last
    2r columns (corners included) exhaustive; one chunk per row for 1 and 2 channels (both row ends on one lane)."""
    torch = torch_cuda
    for c in range(1, 5):
        mask = torch.from_numpy(kp.edge_mask_np(r, c)).cuda()
        assert mask.shape[0] == kp.edge_combos(r) and mask.shape[2] >= 4 * r
        check_two_valued(pkg, L, torch, mask, r, f"edges r={r} C={c}")
        del mask
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- generic median: the rank boundary
def test_median_generic_rank_boundary(pkg, L, torch_cuda):
    """Two-valued images of every (v, v+1) and every (0, v), high with density (K + 0.5) / N so that every image has
    windows with exactly K and exactly K+1 high values: the bit-serial select keeps a bit exactly when at most K values
    lie below it."""
    torch = torch_cuda
    pairs = [(v, v + 1) for v in range(255)] + [(0, v) for v in range(1, 256)]
    lo = np.array([p[0] for p in pairs], np.uint8)[:, None, None, None]
    hi = np.array([p[1] for p in pairs], np.uint8)[:, None, None, None]
    rng = np.random.default_rng(77)
    for r in range(1, 8):
        n, k = (2 * r + 1) ** 2, ((2 * r + 1) ** 2 - 1) // 2
        routes = [(1, 0)] if r > 2 else [(5, 0), (1, 1)]           # (channels, input offset): radius 1 | 2 off the fast path
        for c, off in routes:
            mask = (rng.random((len(pairs), 24, 32, c)) < (k + 0.5) / n).astype(np.uint8)
            cnt = kp.high_count_np(mask, r)
            on_k, on_k1 = (cnt == k).any(axis=(1, 2, 3)), (cnt == k + 1).any(axis=(1, 2, 3))
            assert on_k.all() and on_k1.all(), (r, c)
            img = np.where(mask.astype(bool), hi, lo)
            got = median_dev(pkg, L, torch, torch.from_numpy(img).cuda(), r, offset_in=off).cpu().numpy()
            assert L.mi_blur_last_kernel() == GENERIC, (r, c, off)
            want = kp.ref_median(img, r)
            assert np.array_equal(want, kp.median_from_count(cnt, r, lo, hi)), r
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (r, c, off, len(bad), pairs[bad[0][0]])


# ---------------------------------------------------------------- separable tiled kernel: geometry and taps
SEP_CPR = (1, 2, 3, 31, 32, 33, 64, 65, 97)
SEP_ROWS = (1, 2, 7, 8, 9, 31, 32, 33, 64, 65)
SEP_RX = (0, 4, 5, 8, 9, 16)
SEP_RY = (0, 1, 8, 16)


def test_sep_tiled_geometry_sweep(pkg, L, torch_cuda):
    """Every chunk count x every row count for 1..4 channels; (rx, ry) walk through all 24 bucket-edge pairs."""
    torch = torch_cuda
    rng = np.random.default_rng(31)
    for c in range(1, 5):
        seen = set()
        for i, cpr in enumerate(SEP_CPR):
            w = kp.chunk_cols(cpr, c) * 16 // c
            for j, rows in enumerate(SEP_ROWS):
                q = i * len(SEP_ROWS) + j
                rx, ry = SEP_RX[q % 6], SEP_RY[(q // 6) % 4]
                seen.add((rx, ry))
                wx, wy = kp.rand_taps(rng, rx, int(rng.integers(0, 9))), kp.rand_taps(rng, ry, int(rng.integers(0, 9)))
                img = rng.integers(0, 256, size=(1, rows, w, c), dtype=np.uint8)
                got = sep_dev(pkg, L, torch, torch.from_numpy(img).cuda(), wx, wy).cpu().numpy()
                assert L.mi_blur_last_kernel() == TILED, (c, cpr, rows)
                assert np.array_equal(got, kp.ref_sep(img, wx, wy)), (c, cpr, rows, wx, wy)
        assert len(seen) == 24, c


def sep_taps(pkg, rx, ry):
    return lambda rng: pkg.SepKernel.from_taps(kp.rand_taps(rng, rx, 8), kp.rand_taps(rng, ry, 8))


def test_sep_tiled_bands_and_grids(pkg, L, torch_cuda):
    """Bands whose y0 / y1 sit on and next to tile boundaries (multiples of 32); batches whose grid is below and at or
    above 16 blocks (the XCD remap off and on)."""
    check_bands_and_grids(SEP, pkg, L, torch_cuda, np.random.default_rng(32), random_bytes,
                          [sep_taps(pkg, rx, ry) for rx, ry in ((1, 16), (8, 3), (16, 9))], sep_taps(pkg, 5, 4))


def test_sep_tiled_one_hot_taps(pkg, L, torch_cuda):
    """A tap 2^b at offset d, for every d of every radius bucket (each one its own byte-offset instantiation of the
    horizontal pass) and likewise vertically: the image moved by d, clamped."""
    torch = torch_cuda
    rng = np.random.default_rng(33)
    imgs = {}
    for c, axis, rb, d, b, w, h in kp.one_hot_cases():
        if (c, w, h) not in imgs:
            img = rng.integers(0, 256, size=(1, h, w, c), dtype=np.uint8)
            imgs[(c, w, h)] = (img, torch.from_numpy(img).cuda())
        img, d_img = imgs[(c, w, h)]
        t = kp.one_hot(rb, d, b)
        wx, wy = (t, [1]) if axis == 2 else ([1], t)
        got = sep_dev(pkg, L, torch, d_img, wx, wy).cpu().numpy()
        assert L.mi_blur_last_kernel() == TILED
        want = kp.shifted(img, d, axis)
        assert np.array_equal(want, kp.ref_sep(img, wx, wy)), (c, axis, rb, d, b)
        assert np.array_equal(got, want), (c, axis, rb, d, b, w)


# ---------------------------------------------------------------- median fast kernel: geometry
MED_CPR = (1, 2, 61, 62, 63, 64, 123, 124, 125, 248, 249)


def med_nblocks(n, rows, cpr, r):
    total = n * ((rows + kp.med_bh(r) - 1) // kp.med_bh(r)) * cpr
    return ((total + 61) // 62 + 3) // 4


def test_median_fast_geometry_sweep(pkg, L, torch_cuda):
    """Chunk counts around the 62 computing lanes of a wave (and two, four waves), rows around the lane's band of BH,
    one and three images, grids below and at or above 16 blocks."""
    torch = torch_cuda
    rng = np.random.default_rng(41)
    for r in (1, 2):
        bh = kp.med_bh(r)
        for c in range(1, 5):
            sides = set()
            cases = [(1 + 2 * ((i + j) % 2), rows, cpr) for i, cpr in enumerate(MED_CPR)
                     for j, rows in enumerate((1, bh - 1, bh, bh + 1, 2 * bh + 1))]
            cases += [(4, 2 * bh + 1, 249), (5, 2 * bh + 1, 249)]      # 13 and 16 blocks
            for n, rows, cpr in cases:
                cc = kp.chunk_cols(cpr, c)
                sides.add(med_nblocks(n, rows, cc, r) >= 16)
                img = rng.integers(0, 256, size=(n, rows, cc * 16 // c, c), dtype=np.uint8)
                got = median_dev(pkg, L, torch, torch.from_numpy(img).cuda(), r).cpu().numpy()
                assert L.mi_blur_last_kernel() == FAST, (r, c, n, rows, cpr)
                assert np.array_equal(got, kp.ref_median(img, r)), (r, c, n, rows, cpr)
            assert sides == {False, True}, (r, c)


def test_median_fast_bands(pkg, L, torch_cuda):
    """Bands whose y0 / y1 sit on and next to multiples of BH."""
    torch = torch_cuda
    rng = np.random.default_rng(42)
    for r in (1, 2):
        bh = kp.med_bh(r)
        h = 4 * bh + 3
        for c in range(1, 5):
            for cpr in (1, 62):
                cc = kp.chunk_cols(cpr, c)
                img = rng.integers(0, 256, size=(1, h, cc * 16 // c, c), dtype=np.uint8)
                d_img = torch.from_numpy(img).cuda()
                whole = kp.ref_median(img, r)
                for y0 in (0, 1, bh - 1, bh, bh + 1, 2 * bh):
                    for y1 in sorted({y0 + 1, 2 * bh, 2 * bh + 1, 3 * bh - 1, h} - set(range(y0 + 1))):
                        got = median_dev(pkg, L, torch, d_img, r, y0, y1).cpu().numpy()
                        assert L.mi_blur_last_kernel() == FAST, (r, c, y0, y1)
                        assert np.array_equal(got, whole[:, y0:y1]), (r, c, cpr, y0, y1)


# ---------------------------------------------------------------- the morph proof (window positions)
def test_morph_tiled_proof_every_window_position(pkg, L, torch_cuda):
    """The proof images at every radius 0..16 on the proved axis (the other at 0), then (3, 3), (4, 4) and (16, 16), for
    1..4 channels and all three ops: an output whose window lacked a source byte, or held one too many, at any byte
    position of the horizontal pass's two chunks or any row of the vertical pass's group, differs from the restatement."""
    torch = torch_cuda
    for axis in (2, 1):
        for c in kp.MORPH_PROOF_C:
            img = mr.proof_horizontal(c) if axis == 2 else mr.proof_vertical(c)
            d_img = torch.from_numpy(img).cuda()
            for rx, ry in kp.morph_proof_cases(axis):
                lo, hi = (torch.from_numpy(a).cuda() for a in mr.ref_lo_hi(img, rx, ry))
                for op, want in ((mr.ERODE, lo), (mr.DILATE, hi), (mr.GRADIENT, hi - lo)):
                    got = dev_run(MORPH, pkg, L, torch, d_img, (op, rx, ry))
                    assert L.mi_blur_last_kernel().decode() == MORPH.fast, (axis, c, op, rx, ry)
                    assert_same(torch, got, want, f"morph axis={axis} C={c} op={op} rx={rx} ry={ry}")


# ---------------------------------------------------------------- morph, bilateral, conv: geometry, bands, grids
MORPH_RX = (0, 1, 4, 5, 8, 11, 16)        # morph_hc(C, rx) = ceil(rx C / 16), at least 1, changes along this list for every C > 1
MORPH_RY = (0, 3, 4, 16)                  # straight taps up to 3, van Herk from 4
CONV_RY = (0, 1, 7)


def morph_filter(q):
    rx, ry = MORPH_RX[q % 7], MORPH_RY[(q // 7) % 4]
    return (mr.OPS[q % 3], rx, ry), (rx, ry)


def bilateral_filter(pkg):
    def make(q):
        r = 1 + q % 8
        return pkg.Bilateral.gauss(0.0, 10.0 + 5.0 * (q % 7), r), r
    return make


def conv_filter(pkg, rng):
    def make(q):
        rx, ry = q % 8, CONV_RY[(q // 8) % 3]                      # rx 0..7: all five column classes of blur_conv_tiled_kernel
        return cr.make_kernel(pkg, **cr.random_kernel(rng, rx, ry, mode=cr.MODES[q % 3])), (rx, ry)
    return make


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_morph_tiled_geometry_sweep(pkg, L, torch_cuda, c):
    check_tiled_geometry_sweep(MORPH, pkg, L, torch_cuda, np.random.default_rng(50 + c), c, mr.mixed, morph_filter, 28)


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_bilateral_tiled_geometry_sweep(pkg, L, torch_cuda, c):
    check_tiled_geometry_sweep(BILATERAL, pkg, L, torch_cuda, np.random.default_rng(60 + c), c, random_bytes, bilateral_filter(pkg), 8)


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_conv_tiled_geometry_sweep(pkg, L, torch_cuda, c):
    rng = np.random.default_rng(70 + c)
    check_tiled_geometry_sweep(CONV, pkg, L, torch_cuda, rng, c, random_bytes, conv_filter(pkg, rng), 24)


def test_morph_tiled_bands_and_grids(pkg, L, torch_cuda):
    check_bands_and_grids(MORPH, pkg, L, torch_cuda, np.random.default_rng(51), mr.mixed,
                          [lambda rng, f=f: f for f in ((mr.ERODE, 1, 16), (mr.DILATE, 8, 3), (mr.GRADIENT, 16, 9))],
                          lambda rng: (mr.GRADIENT, 5, 4))


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_bilateral_tiled_bands_and_grids(pkg, L, torch_cuda, c):
    check_bands_and_grids(BILATERAL, pkg, L, torch_cuda, np.random.default_rng(61 + c), random_bytes,
                          [lambda rng, r=r: pkg.Bilateral.gauss(0.0, 25.0, r) for r in (1, 8)],
                          lambda rng: pkg.Bilateral.gauss(0.0, 25.0, 2), channels=(c,))


def test_conv_tiled_bands_and_grids(pkg, L, torch_cuda):
    def conv(rx, ry, mode):
        return lambda rng: cr.make_kernel(pkg, **cr.random_kernel(rng, rx, ry, mode=mode))
    check_bands_and_grids(CONV, pkg, L, torch_cuda, np.random.default_rng(71), random_bytes,
                          [conv(1, 7, "sat"), conv(7, 1, "mag"), conv(4, 3, "abs")], conv(2, 2, "sat"))


# ---------------------------------------------------------------- sep_down: geometry
DOWN_PAIRS = (1, 2, 3, 15, 16, 17, 32, 33, 49)                    # input chunk PAIRS per row: an output row is that many chunks
DOWN_RX = (0, 4, 5, 8, 9, 16)                                     # blur_sep_down_tiled_kernel's radius buckets RB
DOWN_RY = (0, 1, 8, 16)
DOWN_TILED = "blur_sep_down_tiled_kernel"


def test_sep_down_tiled_geometry_sweep(pkg, L, torch_cuda):
    """Every input chunk-pair count (whole groups of three pairs for 3 channels) x every input row count for 1..4
    channels; the four phases cycle and (rx, ry) walk through all 24 bucket-edge pairs."""
    rng = np.random.default_rng(81)
    for c in range(1, 5):
        seen, phases = set(), set()
        for i, pairs in enumerate(DOWN_PAIRS):
            pairs = max(3, int(round(pairs / 3)) * 3) if c == 3 else pairs
            w = pairs * 32 // c
            for j, rows in enumerate(SEP_ROWS):
                q = i * len(SEP_ROWS) + j
                rx, ry = DOWN_RX[q % 6], DOWN_RY[(q // 6) % 4]
                ox, oy = (i + j) % 2, ((i + j) // 2 % 2 if rows > 1 else 0)        # oy < H: the output is never empty
                seen.add((rx, ry))
                phases.add((4 if rx <= 4 else 8 if rx <= 8 else 16, ox, oy))
                wx, wy = kp.rand_taps(rng, rx, int(rng.integers(0, 9))), kp.rand_taps(rng, ry, int(rng.integers(0, 9)))
                img = rng.integers(0, 256, size=(1, rows, w, c), dtype=np.uint8)
                got = rh.gpu_run(rh.SEP_DOWN, pkg, L, torch_cuda, img, (pkg.SepKernel.from_taps(wx, wy), (2, 2, ox, oy)))
                assert L.mi_blur_last_kernel().decode() == DOWN_TILED, (c, pairs, rows)
                assert np.array_equal(got, kp.ref_sep(img, wx, wy)[:, oy::2, ox::2]), (c, pairs, rows, rx, ry, ox, oy)
        assert len(seen) == 24 and len(phases) == 12, c                   # every bucket-edge pair; every phase in every bucket


# ---------------------------------------------------------------- resize: geometry
RESIZE_CI = (1, 2, 3, 31, 32, 33)                                 # input chunks per row
RESIZE_H = (1, 2, 31, 32, 33)
RESIZE_TILED = "blur_resize_tiled_kernel"


def resize_x_cases(c):
    """(input chunks, output chunks): each input count with the counts at and next to 1x, 2x, 3x and 97, kept where the
    output row is at least as wide as the input row (after rounding both to what whole pixels of c channels fill)."""
    out = []
    for ci in RESIZE_CI:
        a = kp.chunk_cols(ci, c)
        for co in (ci, ci + 1, 2 * ci - 1, 2 * ci, 2 * ci + 1, 3 * ci + 1, 97):
            b = kp.chunk_cols(co, c)
            if b >= a and (a, b) not in out:
                out.append((a, b))
    return out


def resize_y_cases():
    out = []
    for h in RESIZE_H:
        for ho in (h, h + 1, 2 * h - 1, 2 * h, 2 * h + 1, 32 * h + 1):
            if ho >= h and (h, ho) not in out:
                out.append((h, ho))
    return out


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_resize_tiled_geometry_sweep(pkg, L, torch_cuda, c):
    """The x cases and the y cases paired cyclically (every one of either list occurs), through the tiled kernel."""
    rng = np.random.default_rng(90 + c)
    xs, ys = resize_x_cases(c), resize_y_cases()
    used_x, used_y = set(), set()
    for k in range(max(len(xs), len(ys))):
        (ci, co), (h, ho) = xs[k % len(xs)], ys[(k + c) % len(ys)]
        used_x.add((ci, co))
        used_y.add((h, ho))
        w, wo = ci * 16 // c, co * 16 // c
        img = rng.integers(0, 256, size=(1, h, w, c), dtype=np.uint8)
        assert takes_tiled(img.shape, wo, ho), (c, ci, co, h, ho)
        got = rh.gpu_run(rh.RESIZE, pkg, L, torch_cuda, img, (wo, ho, BILINEAR))
        assert L.mi_blur_last_kernel().decode() == RESIZE_TILED, (c, ci, co, h, ho)
        assert np.array_equal(got, ref_resize(img, wo, ho)), (c, ci, co, h, ho)
    assert len(used_x) == len(xs) and len(used_y) == len(ys)


# ---------------------------------------------------------------- warp: geometry
WARP_WO = (16, 48, 64, 80, 128, 144)      # output pixels per row: whole chunks (groups of three for 3 channels) for 1..4 channels; one strip, its 64-pixel edge, at and next to two strips
WARP_HO = (1, 2, 31, 32, 33, 65)
WARP_IN = (80, 96)                        # input rows, pixels per row
WARP_TILED = "blur_warp_tiled_kernel"


def warp_maps():
    """(m, borders): a sub-pixel translation, a rotation by 30 degrees about the centre, the x2 CLAMP scale, a x1/2
    reduction, and a translation that puts the tiles on the right and at the bottom wholly outside the image."""
    h, w = WARP_IN
    both = (wr.CLAMP, wr.CONSTANT)
    return [([wr.Q, 0, 3 * wr.Q // 8 + 1, 0, wr.Q, -5 * wr.Q // 8 - 1], both), (wr.rotation_m(w, h, 30.0), both), (wr.scale_matrix(2, 1), both),
            (wr.scale_matrix(1, 2), both), ([wr.Q, 0, 40 * wr.Q + 123, 0, wr.Q, 45 * wr.Q - 77], both)]


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_warp_tiled_geometry_sweep(pkg, L, torch_cuda, c):
    """Every output width x every output height paired cyclically (every one of either list occurs), each under every map
    and both borders, through the tiled kernel, byte for byte against warp_ref.ref_warp."""
    h, w = WARP_IN
    img = np.random.default_rng(100 + c).integers(0, 256, size=(1, h, w, c), dtype=np.uint8)
    used_w, used_h, missed = set(), set(), False
    for k in range(max(len(WARP_WO), len(WARP_HO))):
        wo, ho = WARP_WO[k % len(WARP_WO)], WARP_HO[(k + c) % len(WARP_HO)]
        used_w.add(wo)
        used_h.add(ho)
        for i, (m, borders) in enumerate(warp_maps()):
            for border in borders:
                assert wr.takes_tiled(img.shape, m, wo, ho, wr.BILINEAR, border), (c, wo, ho, i, border)
                got = rh.gpu_run(rh.WARP, pkg, L, torch_cuda, img, (m, wo, ho, wr.BILINEAR, border, 201))
                assert L.mi_blur_last_kernel().decode() == WARP_TILED, (c, wo, ho, i, border)
                want = wr.ref_warp(img, m, wo, ho, wr.BILINEAR, border, 201)
                assert np.array_equal(got, want), (c, wo, ho, i, border)
                if i == 4 and border == wr.CONSTANT:
                    ncols, cpr, trows = wr.tile_geometry(wo, ho, c)
                    missed = missed or any(wr.footprint(m, border, w, h, c, x0c * 16 // c, (min(x0c + ncols, cpr) * 16 - 1) // c, ty0, min(ty0 + trows, ho) - 1) == 0
                                           for ty0 in range(0, ho, trows) for x0c in range(0, cpr, ncols))
    assert len(used_w) == len(WARP_WO) and len(used_h) == len(WARP_HO)
    assert missed                                                      # some tile lay wholly outside the image
