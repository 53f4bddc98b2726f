"""The distance transform on the GPU (mi_blur_enqueue_dist, mi_blur_enqueue_dist_u8, distance_transform() and its kin on
device 0): word for word and byte for byte against the CPU device, and against dist_ref.py on the small cases, inside
guard patterns, and which kernel took each launch."""
import ctypes as C

import numpy as np
import pytest

import dist_ref as R
from large_harness import BAND as CMP_BAND
from large_harness import BASE, bands_of
from resample_harness import last, torch_cuda  # noqa: F401
from table_harness import Guarded, stream, upload

pytestmark = pytest.mark.gpu

GUARD = 16                                    # words in front of a table (64 bytes: the table stays 16-byte aligned) and behind it
B = R.BAND
CAP = 16384 * 256                             # byte_grid(), csrc/kernel_common.h: workgroups x threads


def work_buffer(pkg, L, torch, shape, k, band=B):
    n, h, w, c = shape
    nwork = L.mi_blur_dist_work_bytes(w, h, c, n, C.byref(k))
    assert nwork == R.work_bytes(shape, band)
    return Guarded(torch, nwork, "the work buffer")


def gpu_table(pkg, L, torch, img, k, band=B):
    """mi_blur_enqueue_dist: the table inside 0xFFFFFFFF words, the work buffer with 64 bytes of 0x5A behind it."""
    n, h, w, c = img.shape
    d_in, p_in = upload(torch, img)
    buf = Guarded(torch, img.size, "the table", np.uint32, 0xFFFFFFFF, GUARD, GUARD)
    d_work = work_buffer(pkg, L, torch, img.shape, k, band)
    pkg.check(L.mi_blur_enqueue_dist(p_in, buf.ptr, w, h, c, n, C.byref(k), d_work.ptr, stream(torch)), "mi_blur_enqueue_dist")
    torch.cuda.synchronize()
    d_work.payload()
    assert bool((d_in == upload(torch, img)[0]).all()), "wrote to the input"
    return buf.payload().reshape(img.shape)


def gpu_bytes(pkg, L, torch, img, k, offset_out=0, in_place=False, band=B):
    """mi_blur_enqueue_dist_u8: the output offset_out bytes into a buffer of 0x5A with 128 bytes to spare, or the input itself."""
    n, h, w, c = img.shape
    d_in, p_in = upload(torch, img)
    d_out = Guarded(torch, img.size, "the output", front=offset_out, back=128 - offset_out)
    d_work = work_buffer(pkg, L, torch, img.shape, k, band)
    pkg.check(L.mi_blur_enqueue_dist_u8(p_in, d_out.ptr if not in_place else p_in, w, h, c, n, C.byref(k), d_work.ptr, stream(torch)), "mi_blur_enqueue_dist_u8")
    torch.cuda.synchronize()
    d_work.payload()
    if in_place:
        assert bool((d_out.tensor == 0x5A).all())
        return d_in[:img.size].cpu().numpy().reshape(img.shape)
    return d_out.payload().reshape(img.shape)


def cpu_table(pkg, L, img, k):
    out = np.empty(img.shape, np.uint32)
    n, h, w, c = img.shape
    pkg.check(L.mi_blur_cpu_run_dist(img.ctypes.data, out.ctypes.data, w, h, c, n, C.byref(k), 4), "mi_blur_cpu_run_dist")
    return out


def check(pkg, L, torch, img, metric, nonzero=0, limit=0, ref=None, band=B, offset_out=0):
    """The table against the CPU device (and `ref` of dist_ref.py), the byte form and, with a limit, both WITHIN forms against
    dist_ref.py's bytes of that table, each in the kernel the header's rule names; the table."""
    img = np.ascontiguousarray(img)
    kt = pkg.Dist(metric, nonzero, limit, 0, 0)
    want = cpu_table(pkg, L, img, kt)
    if ref is not None:
        assert np.array_equal(want, ref(img, metric, nonzero, limit)), (img.shape, metric, limit)
    got = gpu_table(pkg, L, torch, img, kt, band)
    assert last(L) == (R.TILED if R.takes_tiled(img.shape) else R.GENERIC), img.shape
    assert np.array_equal(got, want), (img.shape, metric, nonzero, limit)
    for kb in (pkg.Dist(metric, nonzero, limit, R.BYTE, 0),) + ((pkg.Dist(metric, nonzero, limit, R.WITHIN, 0), pkg.Dist(metric, nonzero, limit, R.WITHIN, 1)) if limit else ()):
        b = gpu_bytes(pkg, L, torch, img, kb, offset_out, band=band)
        assert last(L) == (R.TILED if R.takes_tiled(img.shape, offset_out) else R.GENERIC), (img.shape, offset_out)
        assert np.array_equal(b, R.ref_bytes(want, metric, kb.byte_op, kb.invert)), (img.shape, metric, limit, kb.byte_op, kb.invert)
    return got


def random_sites(rng, shape, density):
    img = rng.integers(1, 256, size=shape, dtype=np.uint8)
    img[rng.random(shape) < density] = 0
    return img


def one_site(shape, sites):
    img = np.full(shape, 255, np.uint8)
    for s in sites:
        img[s] = 0
    return img


# ---------------------------------------------------------------- the column pass: band carries
def carry_image(h, w, c):
    """Per column (and channel) one pattern in turn: the only site in row 0, in row h - 1, in a middle row, none, both ends."""
    img = np.full((2, h, w, c), 255, np.uint8)
    for e in range(w * c):
        x, ch, kind = e // c, e % c, e % 5
        rows = {0: [0], 1: [h - 1], 2: [h // 2], 3: [], 4: [0, h - 1]}[kind]
        for y in rows:
            img[0, y, x, ch] = 0
            img[1, h - 1 - y, (x + 1) % w, ch] = 0
    return img


@pytest.mark.parametrize("metric", R.METRICS)
def test_band_carries(pkg, L, torch_cuda, metric):
    """Bands of 4 rows: carries cross two and more bands both ways and pass through bands without a site; then the default band."""
    try:
        assert L.mi_blur_set_option(b"dist_band", 4) == pkg.OK
        for h in (3, 4, 5, 9, 13):
            for w, c in ((8, 1), (5, 3)):
                check(pkg, L, torch_cuda, carry_image(h, w, c), metric, ref=R.ref_brute, band=4)
    finally:
        assert L.mi_blur_set_option(b"dist_band", B) == pkg.OK
    for h in (B - 1, B, B + 1, 2 * B + 1):
        check(pkg, L, torch_cuda, carry_image(h, 8, 1), metric, ref=R.ref_brute)
        check(pkg, L, torch_cuda, carry_image(h, 3, 2), metric, nonzero=1, ref=R.ref_brute)


# ---------------------------------------------------------------- the row pass: width edges and the two kernels
@pytest.mark.parametrize("c", [1, 3])
def test_width_edges(pkg, L, torch_cuda, c):
    rng = np.random.default_rng(400 + c)
    widths = [1, 8, 15, 16, 17, 24, 31, 32, 33, 63, 64, 65, 257]
    assert {w for w in widths if R.takes_tiled((1, 1, w, c))} == {8, 16, 24, 32, 64}
    for w in widths:
        for density in (0.02, 0.3):
            img = random_sites(rng, (2, 11, w, c), density)
            for metric in R.METRICS:
                check(pkg, L, torch_cuda, img, metric, ref=R.ref_separable)
    img = random_sites(rng, (2, 11, 64, c), 0.02)                              # an output pointer off 16 bytes: the generic kernel
    for off in (1, 8):
        assert R.takes_tiled(img.shape) and not R.takes_tiled(img.shape, off)
        check(pkg, L, torch_cuda, img, R.L2, offset_out=off)


def test_rows_per_workgroup_and_the_widest_rows(pkg, L, torch_cuda):
    """W * C either side of every step of dist_rows(), with 11 rows and two images (a workgroup's rows span the images),
    and either side of the tiled kernel's widest row."""
    rng = np.random.default_rng(410)
    assert [R.rows_per_group((1, 1, w, 1)) for w in (8, 512, 520, 1360, 1368, 2048, 2056, 4096)] == [8, 8, 7, 3, 2, 2, 1, 1]
    for w in (512, 520, 1368, 2048, 2056):
        check(pkg, L, torch_cuda, random_sites(rng, (2, 11, w, 1), 0.004), R.L2)
    check(pkg, L, torch_cuda, random_sites(rng, (2, 11, 130, 4), 0.01), R.L1)
    for wc in (R.MAX_ROW - 8, R.MAX_ROW, R.MAX_ROW + 8):
        for c in (1, 3, 4) if wc == R.MAX_ROW else (1,):
            img = random_sites(rng, (1, 3, wc // c, c), 0.0005)
            assert R.takes_tiled(img.shape) == (wc <= R.MAX_ROW)
            check(pkg, L, torch_cuda, img, R.L2)
    check(pkg, L, torch_cuda, random_sites(rng, (1, 2, R.MAX_ROW, 1), 0.0005), R.LINF, limit=40)


def test_chunk_skipping(pkg, L, torch_cuda):
    """The nearest site several chunks away past chunks that cannot beat it; a far chunk that wins by one over the own
    column's offer; both for every metric, in the tiled and (one column more) the generic kernel, and with the other chunk sizes."""
    for w in (256, 257):
        img = one_site((1, 40, w, 1), [(0, 0, 5, 0), (0, 0, 159, 0), (0, 39, 180, 0)])
        for metric in R.METRICS:
            got = check(pkg, L, torch_cuda, img, metric, ref=R.ref_brute)
            assert got[0, 0, 60, 0] == R.combine(metric, 55, 0)                     # three chunks to the left, past empty ones
        # (170, 0): (159, 0) wins with 121; the chunk to the right is nearer than that (6 columns) but its minimum, 39 rows, cannot
        assert check(pkg, L, torch_cuda, img, R.L2, ref=R.ref_brute)[0, 0, 170, 0] == 121
        img = one_site((1, 16, w, 1), [(0, 13, 101, 0), (0, 1, 112, 0)])
        assert check(pkg, L, torch_cuda, img, R.L2, ref=R.ref_brute)[0, 1, 100, 0] == 144 == 12 ** 2 + 1 ** 2 - 1   # (112, 1) over (101, 13)
        img = one_site((1, 16, w, 1), [(0, 8, 97, 0), (0, 1, 112 - 3, 0), (0, 1, 94, 0)])
        assert check(pkg, L, torch_cuda, img, R.L1, ref=R.ref_brute)[0, 1, 100, 0] == 6                 # (94, 1): the chunk to the left
        img = one_site((1, 16, w, 1), [(0, 14, 100, 0), (0, 1, 112, 0)])
        assert check(pkg, L, torch_cuda, img, R.LINF, ref=R.ref_brute)[0, 1, 100, 0] == 12 == 13 - 1
    rng = np.random.default_rng(420)
    img = random_sites(rng, (2, 9, 200, 3), 0.003)
    try:
        for log2 in (3, 5):
            assert L.mi_blur_set_option(b"dist_chunk_log2", log2) == pkg.OK
            for metric in R.METRICS:
                check(pkg, L, torch_cuda, img, metric, ref=R.ref_separable)
            check(pkg, L, torch_cuda, random_sites(rng, (1, 2, R.MAX_ROW // 4, 4), 0.0005), R.L2)
    finally:
        assert L.mi_blur_set_option(b"dist_chunk_log2", R.CHUNK.bit_length() - 1) == pkg.OK


# ---------------------------------------------------------------- the marker, the limit, channels and batch
@pytest.mark.parametrize("metric", R.METRICS)
def test_the_none_marker(pkg, L, torch_cuda, metric):
    """One column of sites in a wide image, every other column empty; and no site at all: table and both byte forms."""
    img = np.full((1, 8, 1024, 1), 7, np.uint8)
    img[0, :, 777, 0] = 0
    got = check(pkg, L, torch_cuda, img, metric, ref=R.ref_separable)
    assert got[0, 3, 0, 0] == R.combine(metric, 777, 0) and got[0, 3, 1023, 0] == R.combine(metric, 246, 0)
    check(pkg, L, torch_cuda, img[:, :, :1021], metric, ref=R.ref_separable)        # the generic kernel
    for shape in ((2, 5, 64, 3), (2, 5, 63, 3)):
        empty = np.full(shape, 9, np.uint8)
        for limit in (0, 7):
            assert (check(pkg, L, torch_cuda, empty, metric, limit=limit) == R.NONE).all()
        assert (check(pkg, L, torch_cuda, np.zeros(shape, np.uint8), metric, nonzero=1, limit=3) == R.NONE).all()


def test_limits(pkg, L, torch_cuda):
    rng = np.random.default_rng(430)
    img = random_sites(rng, (1, 64, 96, 3), 0.02)
    for metric in R.METRICS:
        for limit in (1, 5, 300):                                                   # 300: larger than the image
            check(pkg, L, torch_cuda, img, metric, limit=limit, ref=R.ref_separable)
            check(pkg, L, torch_cuda, img[:, :, :95], metric, nonzero=1, limit=limit, ref=R.ref_separable)
    tri = one_site((1, 12, 16, 1), [(0, 2, 3, 0)])
    assert check(pkg, L, torch_cuda, tri, R.L2, limit=5, ref=R.ref_brute)[0, 6, 6, 0] == 25
    assert check(pkg, L, torch_cuda, tri, R.L2, limit=4, ref=R.ref_brute)[0, 6, 6, 0] == R.NONE
    assert check(pkg, L, torch_cuda, tri[:, :, :13], R.L2, limit=5, ref=R.ref_brute)[0, 6, 6, 0] == 25
    assert check(pkg, L, torch_cuda, tri[:, :, :13], R.L2, limit=4, ref=R.ref_brute)[0, 6, 6, 0] == R.NONE


def test_channels_and_batch(pkg, L, torch_cuda):
    rng = np.random.default_rng(440)
    for c in (1, 2, 3, 4):
        for w in (40, 37):
            img = np.full((3, 21, w, c), 200, np.uint8)
            for ch in range(c):                                                     # other sites in every channel and image; image 1 empty
                for i in (0, 2):
                    ys, xs = rng.integers(0, 21, 3), rng.integers(0, w, 3)
                    img[i, ys, xs, ch] = 0
            for metric in R.METRICS:
                got = check(pkg, L, torch_cuda, img, metric, ref=R.ref_brute)
                assert (got[1] == R.NONE).all() and (got[0] != R.NONE).all()


@pytest.mark.parametrize("shape", [(1, 1, 32768, 1), (1, 32768, 1, 1), (1, 32768, 8, 1)])
def test_extremes(pkg, L, torch_cuda, shape):
    """The longest row (beyond the tiled bound: the generic kernel at its widest), the longest column, and eight columns of
    32768 rows in the tiled kernel: the only site in a corner, so the far end holds 32767^2 (+ 49)."""
    n, h, w, c = shape
    assert R.takes_tiled(shape) == (w == 8)
    img = one_site(shape, [(0, 0, 0, 0)])
    ys, xs = np.arange(h, dtype=np.int64).reshape(h, 1), np.arange(w, dtype=np.int64).reshape(1, w)
    for metric in R.METRICS:
        got = check(pkg, L, torch_cuda, img, metric)
        assert np.array_equal(got[0, :, :, 0], R.combine(metric, xs + 0 * ys, ys + 0 * xs).astype(np.uint32))
    assert int(check(pkg, L, torch_cuda, img, R.L2, limit=32767)[0, h - 1, w - 1, 0]) == (32767 ** 2 if w * h == 32768 else R.NONE)


def test_generic_kernel_past_its_grid_cap(pkg, L, torch_cuda):
    """blur_dist_generic_kernel strides under byte_grid(): on the base shape every thread makes two trips and 1525 a third.
    The whole output against the CPU device; with the limit 6 a band of rows depends on 6 rows either side only, so the
    bands around the trip boundaries are restated from their slabs."""
    n, h, w, c = BASE
    assert n * h * w * c == 2 * CAP + 1525 and not R.takes_tiled(BASE)
    img = random_sites(np.random.default_rng(450), BASE, 0.01)
    limit = 6
    got = check(pkg, L, torch_cuda, img, R.L2, limit=limit)
    for i, r0 in bands_of(BASE, (CAP, 2 * CAP)):
        lo, hi = max(r0 - limit, 0), min(r0 + CMP_BAND + limit, h)
        slab = R.ref_separable(np.ascontiguousarray(img[i:i + 1, lo:hi]), R.L2, 0, limit)
        assert np.array_equal(got[i, r0:r0 + CMP_BAND], slab[0, r0 - lo:r0 - lo + CMP_BAND]), (i, r0)


def test_in_place(pkg, L, torch_cuda):
    rng = np.random.default_rng(460)
    for shape, kernel in (((2, 40, 48, 3), R.TILED), ((2, 9, 17, 3), R.GENERIC)):
        img = random_sites(rng, shape, 0.01)
        for k in (pkg.Dist(R.L2, 0, 0, R.BYTE, 0), pkg.Dist(R.L1, 1, 9, R.WITHIN, 1)):
            want = R.ref_bytes(R.ref_brute(img, k.metric, k.sites_nonzero, k.limit), k.metric, k.byte_op, k.invert)
            assert np.array_equal(gpu_bytes(pkg, L, torch_cuda, img, k, in_place=True), want) and last(L) == kernel


def test_numpy_functions_on_the_gpu(pkg, L, torch_cuda):
    rng = np.random.default_rng(470)
    mask = np.where(rng.random((3, 90, 128, 3)) < 0.002, 255, 0).astype(np.uint8)
    holes = 255 - mask
    assert np.array_equal(pkg.disc_dilate(mask, 16, "linf", batch=2), pkg.dilate(mask, 33))
    assert np.array_equal(pkg.disc_erode(holes, 16, "linf"), pkg.erode(holes, 33))
    disc = pkg.disc_dilate(mask, 16)
    assert last(L) == R.TILED and np.array_equal(disc, pkg.disc_dilate(mask, 16, device=pkg.DEVICE_CPU))
    odd = mask[0, :45, :71, 0].copy()
    T = pkg.distance_transform(odd, "l2", "nonzero")
    assert last(L) == R.GENERIC and np.array_equal(T, R.ref_brute(odd[None, :, :, None], R.L2, 1)[0, :, :, 0])
    assert np.array_equal(pkg.distance_transform_u8(odd, "l2", "nonzero"), R.ref_bytes(T, R.L2))
    assert np.array_equal(pkg.distance_transform(mask, "l1", "nonzero", 20), pkg.distance_transform(mask, "l1", "nonzero", 20, device=pkg.DEVICE_CPU))
