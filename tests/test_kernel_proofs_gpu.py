"""Kernel proofs and geometry sweeps on a real MI355X (-m gpu), against references computed from the definitions in
include/mi_blur.h (kernel_proofs.py), never from the product; every launch also asserts which kernel ran.

  * blur_median_fast_kernel, all 8 instantiations: exhaustive by the 0-1 principle (kernel_proofs.py).  The interior
    stream puts every two-valued window on every interior row at every byte position its channel can take in a chunk;
    the edge batch enumerates the first and last 2r columns.
  * blur_median_generic_kernel: two-valued images of every adjacent pair (v, v+1) and every (0, v), window counts on K
    and K+1, radius 1..7.
  * blur_sep_tiled_kernel and blur_median_fast_kernel: chunk counts, rows, radius buckets, bands and grids at and next
    to the tile / wave boundaries; one-hot taps at every offset of every radius bucket."""
import ctypes as C
import math

import numpy as np
import pytest

import kernel_proofs as kp
from filter_harness import torch_cuda  # noqa: F401

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
    n, h, w, c = d_img.shape
    k = pkg.SepKernel.from_taps(wx, wy)
    y0 = 0 if y0 is None else y0
    y1 = h if y1 is None else y1
    size = n * (y1 - y0) * w * c
    out = torch.full((size + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if y0 == 0 and y1 == h:
        rc = L.mi_blur_enqueue_sep(d_img.data_ptr(), out.data_ptr() + GUARD, w, h, c, n, C.byref(k), s)
    else:
        assert n == 1
        rc = L.mi_blur_enqueue_sep_band(d_img.data_ptr(), out.data_ptr() + GUARD, w, h, c, y0, y1, C.byref(k), s)
    pkg.check(rc, "mi_blur_enqueue_sep")
    torch.cuda.synchronize()
    assert bool((out[:GUARD] == 0x5A).all()) and bool((out[GUARD + size:] == 0x5A).all()), "wrote outside the output"
    return out[GUARD:GUARD + size].reshape(n, y1 - y0, w, c)


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


def sep_nblocks(n, rows, cpr):
    nstrips = (cpr + 31) // 32
    return n * ((rows + 31) // 32) * nstrips


def test_sep_tiled_bands_and_grids(pkg, L, torch_cuda):
    """Bands whose y0 / y1 sit on and next to tile boundaries (multiples of 32); batches whose grid is below and at or
    above 16 blocks (the XCD remap off and on)."""
    torch = torch_cuda
    rng = np.random.default_rng(32)
    h = 130
    for c in range(1, 5):
        for cpr in (2, 33):
            w = kp.chunk_cols(cpr, c) * 16 // c
            img = rng.integers(0, 256, size=(1, h, w, c), dtype=np.uint8)
            d_img = torch.from_numpy(img).cuda()
            for rx, ry in ((1, 16), (8, 3), (16, 9)):
                wx, wy = kp.rand_taps(rng, rx, 8), kp.rand_taps(rng, ry, 8)
                whole = kp.ref_sep(img, wx, wy)
                for y0 in (0, 1, 31, 32, 33, 63, 64, 65):
                    for y1 in sorted({y0 + 1, 64, 65, 96, 97, h} - set(range(y0 + 1))):
                        got = sep_dev(pkg, L, torch, d_img, wx, wy, y0, y1).cpu().numpy()
                        assert L.mi_blur_last_kernel() == TILED
                        assert np.array_equal(got, whole[:, y0:y1]), (c, cpr, rx, ry, y0, y1)
    sides = set()
    for c in range(1, 5):
        for n, rows, cpr in ((2, 32, 32), (15, 32, 32), (16, 32, 32), (3, 65, 65), (5, 33, 1), (9, 31, 33)):
            w = kp.chunk_cols(cpr, c) * 16 // c
            nb = sep_nblocks(n, rows, kp.chunk_cols(cpr, c))
            sides.add((c, nb >= 16))
            img = rng.integers(0, 256, size=(n, rows, w, c), dtype=np.uint8)
            wx, wy = kp.rand_taps(rng, 5, 8), kp.rand_taps(rng, 4, 8)
            got = sep_dev(pkg, L, torch, torch.from_numpy(img).cuda(), wx, wy).cpu().numpy()
            assert L.mi_blur_last_kernel() == TILED
            assert np.array_equal(got, kp.ref_sep(img, wx, wy)), (c, n, rows, cpr, nb)
    assert len(sides) == 8


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
