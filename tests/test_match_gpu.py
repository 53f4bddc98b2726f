"""Template matching and the peak search on the GPU (mi_blur_enqueue_match, mi_blur_enqueue_match_peak and the Python
functions on device 0): word for word against the CPU device and, on the small shapes, against match_ref.py, every output
and work buffer inside guard patterns, and which kernel took each launch."""
import ctypes as C

import numpy as np
import pytest

import match_ref as R
from resample_harness import last, torch_cuda  # noqa: F401
from table_harness import Guarded, stream, upload
from test_match_host import cpu_match, cpu_peak

pytestmark = pytest.mark.gpu

GUARD = 16                                    # words around a table: it stays 16-byte aligned
TX, TY = R.TILE                               # blur_match_tiled_kernel's tile (csrc/filter.h: MATCH_TX, MATCH_TY)
CAP = 16384 * 256                             # byte_grid(), csrc/kernel_common.h: workgroups x threads
TILED, GENERIC = "blur_match_tiled_kernel", "blur_match_generic_kernel"


def gpu_match(pkg, L, torch, img, t, method, offset_in=0):
    """mi_blur_enqueue_match: the table inside 0xFFFFFFFF words, the work buffer with 64 bytes of 0x5A behind it."""
    n, h, w, c = img.shape
    shared = t.ndim == 3
    th, tw = t.shape[-3], t.shape[-2]
    k = pkg.Match(method, tw, th, int(shared))
    d_in, p_in = upload(torch, img, offset_in)
    d_t, p_t = upload(torch, t)
    entries = n * (h - th + 1) * (w - tw + 1)
    buf = Guarded(torch, entries, "the table", np.uint32, 0xFFFFFFFF, GUARD, GUARD)
    nwork = L.mi_blur_match_work_bytes(w, h, c, n, C.byref(k))
    assert nwork > 0
    d_work = Guarded(torch, nwork, "the work buffer")
    pkg.check(L.mi_blur_enqueue_match(p_in, p_t, buf.ptr, w, h, c, n, C.byref(k), d_work.ptr, stream(torch)), "mi_blur_enqueue_match")
    torch.cuda.synchronize()
    d_work.payload()
    assert bool((d_in == upload(torch, img, offset_in)[0]).all()) and bool((d_t == upload(torch, t)[0]).all()), "wrote to an input"
    out = buf.payload().reshape(n, h - th + 1, w - tw + 1)
    return out.view(np.int32) if method >= R.NCC else out


def gpu_peak(pkg, L, torch, table):
    n, ho, wo = table.shape
    d_t, p_t = upload(torch, table)
    peaks = Guarded(torch, n * 12, "the peaks", np.uint32, 0xFFFFFFFF, GUARD, GUARD)
    nwork = L.mi_blur_match_peak_work_bytes(wo, ho, n)
    d_work = Guarded(torch, nwork, "the work buffer")
    pkg.check(L.mi_blur_enqueue_match_peak(p_t, int(table.dtype == np.int32), wo, ho, n, peaks.ptr, d_work.ptr, stream(torch)), "mi_blur_enqueue_match_peak")
    torch.cuda.synchronize()
    d_work.payload()
    return peaks.payload().view(np.int64).reshape(n, 6)


def both_kernels(pkg, L, torch, img, t, method, want_tiled=True):
    """The launch with match_tiled 1 and 0: which kernel took each, and that they agree; the tiled (or only) result."""
    try:
        got = gpu_match(pkg, L, torch, img, t, method)
        raw = method < R.NCC
        if raw:
            assert last(L) == (TILED if want_tiled else GENERIC)
        assert L.mi_blur_set_option(b"match_tiled", 0) == pkg.OK
        plain = gpu_match(pkg, L, torch, img, t, method)
        if raw:
            assert last(L) == GENERIC
    finally:
        assert L.mi_blur_set_option(b"match_tiled", 1) == pkg.OK
    assert np.array_equal(got, plain), "the tiled and the generic kernel differ"
    return got


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_methods_channels_and_batches(pkg, L, torch_cuda, c):
    rng = np.random.default_rng(40 + c)
    img = rng.integers(0, 256, (3, 48, 64, c), dtype=np.uint8)
    widths = {3: (3, 4, 5, 8), 1: (7, 16)}.get(c, (5,))
    for tw in widths:
        for shared in (True, False):
            t = rng.integers(0, 256, (6, tw, c) if shared else (3, 6, tw, c), dtype=np.uint8)
            for method in range(5):
                got = both_kernels(pkg, L, torch_cuda, img, t, method)
                assert np.array_equal(got, cpu_match(pkg, L, img, t, method, 4)), (tw, shared, method)
                if tw == widths[0]:
                    assert np.array_equal(got, R.match(img, t, method)), (tw, shared, method)


@pytest.mark.parametrize("method", [R.SQDIFF, R.CCORR, R.SAD])
def test_tile_edges(pkg, L, torch_cuda, method):
    """Wo and Ho at T - 1, T, T + 1, 2T - 1 and 2T + 1 of the tile.  The template is 5 x 3 wherever the tiled kernel takes
    the row: W * C must be a multiple of 16, so with four channels W = Wo + tw - 1 a multiple of 4, which tw = 5 gives
    for Wo = T only; the other widths take the tw of 2..5 that does (2 for 4j - 1, 4 for 4j + 1)."""
    rng = np.random.default_rng(50 + method)
    for wo in (TX - 1, TX, TX + 1, 2 * TX - 1, 2 * TX + 1):
        tw = {0: 5, 3: 2, 1: 4}[wo % 4]
        for ho in (TY - 1, TY, TY + 1, 2 * TY - 1, 2 * TY + 1):
            img = rng.integers(0, 256, (2, ho + 2, wo + tw - 1, 4), dtype=np.uint8)
            t = rng.integers(0, 256, (3, tw, 4), dtype=np.uint8)
            got = both_kernels(pkg, L, torch_cuda, img, t, method)
            assert got.shape == (2, ho, wo) and np.array_equal(got, cpu_match(pkg, L, img, t, method, 4)), (wo, ho)


def test_template_rows_beyond_one_lds_band(pkg, L, torch_cuda):
    """A template whose input rows do not fit the tile's 48 KiB of LDS at once is walked in bands of template rows:
    200 x 200 x 1 (rows of 272 staged bytes: 165 template rows a band) and 60 x 250 x 4 (496 bytes: 84 rows a band)."""
    rng = np.random.default_rng(61)
    for shape, tshape in (((1, 230, 272, 1), (200, 200, 1)), ((1, 270, 128, 4), (250, 60, 4))):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        t = rng.integers(0, 256, tshape, dtype=np.uint8)
        for method in (R.SQDIFF, R.CCORR, R.SAD):
            assert np.array_equal(both_kernels(pkg, L, torch_cuda, img, t, method), cpu_match(pkg, L, img, t, method, 8)), (shape, method)


def test_misaligned_input_and_odd_widths(pkg, L, torch_cuda):
    rng = np.random.default_rng(70)
    t = rng.integers(0, 256, (3, 5, 3), dtype=np.uint8)
    aligned = rng.integers(0, 256, (2, 20, 32, 3), dtype=np.uint8)      # 96 bytes a row
    odd = rng.integers(0, 256, (2, 20, 37, 3), dtype=np.uint8)          # 111 bytes a row
    for method in range(5):
        for img, offset in ((aligned, 1), (odd, 0)):
            got = gpu_match(pkg, L, torch_cuda, img, t, method, offset)
            if method < R.NCC:
                assert last(L) == GENERIC
            assert np.array_equal(got, cpu_match(pkg, L, img, t, method, 2)) and np.array_equal(got, R.match(img, t, method)), (method, offset)
    assert gpu_match(pkg, L, torch_cuda, aligned, t, R.CCORR, 0) is not None and last(L) == TILED


def test_the_ccorr_extremes(pkg, L, torch_cuda):
    img = np.full((1, 129, 130, 4), 255, np.uint8)
    got = both_kernels(pkg, L, torch_cuda, img, np.full((128, 128, 4), 255, np.uint8), R.CCORR, want_tiled=False)      # 520 bytes a row
    assert got.shape == (1, 2, 3) and (got == 4261478400).all()
    img = np.full((1, 129, 132, 4), 255, np.uint8)                      # the same template where the tiled kernel takes the row
    for method, want in ((R.CCORR, 4261478400), (R.SQDIFF, 0), (R.SAD, 0)):
        assert (both_kernels(pkg, L, torch_cuda, img, np.full((128, 128, 4), 255, np.uint8), method) == want).all()
    zeros = np.zeros((128, 128, 4), np.uint8)
    assert (both_kernels(pkg, L, torch_cuda, img, zeros, R.SQDIFF) == 4261478400).all()
    assert (both_kernels(pkg, L, torch_cuda, img, zeros, R.SAD) == 16711680).all()
    rng = np.random.default_rng(71)
    for shape, tshape in (((1, 3, 304, 1), (1, 255, 1)), ((1, 300, 16, 1), (255, 1, 1))):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        t = rng.integers(0, 256, tshape, dtype=np.uint8)
        for method in (R.CCORR, R.SQDIFF, R.SAD, R.ZNCC):
            got = both_kernels(pkg, L, torch_cuda, img, t, method)
            assert np.array_equal(got, cpu_match(pkg, L, img, t, method, 2)) and np.array_equal(got, R.match(img, t, method)), (shape, method)


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(80)
    return rng.integers(0, 256, (1, 2052, 2050, 1), dtype=np.uint8), rng.integers(0, 256, (3, 3, 1), dtype=np.uint8)


@pytest.mark.parametrize("method", [R.SQDIFF, R.CCORR, R.SAD])
def test_generic_kernel_past_its_grid_cap(pkg, L, torch_cuda, big, method):
    """2052 x 2050 x 1 (2050 bytes a row: the generic kernel) with a 3 x 3 template: 2050 x 2048 = 4 198 400 entries, above
    16384 x 256, so the kernel's threads take a second turn.  The CPU device in full, match_ref.py on three bands of 8 rows."""
    img, t = big
    got = gpu_match(pkg, L, torch_cuda, img, t, method)
    assert last(L) == GENERIC and got.size == 4198400 > CAP
    assert np.array_equal(got, cpu_match(pkg, L, img, t, method, 16))
    for y0 in (0, 1021, 2042):
        assert np.array_equal(got[:, y0:y0 + 8], R.match(img[:, y0:y0 + 10], t, method)), y0


def test_scores_on_structured_data(pkg, L, torch_cuda):
    rng = np.random.default_rng(90)
    img = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    x, y = 23, 11
    t = img[y:y + 9, x:x + 12].copy()
    for name in sorted(R.METHODS):
        table = pkg.match_template(img, t, name)
        assert np.array_equal(table, pkg.match_template(img, t, name, pkg.DEVICE_CPU)), name
        assert pkg.find_template(img, t, name) == pkg.find_template(img, t, name, pkg.DEVICE_CPU), name
        assert pkg.find_template(img, t, name)[0] == (x, y), name
        if name in ("sqdiff", "sad"):
            assert table[y, x] == 0 and np.count_nonzero(table == 0) == 1
        if name in ("ncc", "zncc"):
            assert table[y, x] == R.ONE
    flat = np.full((1, 32, 48, 3), 77, np.uint8)
    for method in (R.NCC, R.ZNCC):
        got = both_kernels(pkg, L, torch_cuda, flat, t, method)
        assert (got == 0).all() if method == R.ZNCC else np.array_equal(got, cpu_match(pkg, L, flat, t, method))
    assert (both_kernels(pkg, L, torch_cuda, flat, np.full((4, 4, 3), 9, np.uint8), R.ZNCC) == 0).all()
    tile = rng.integers(0, 256, (8, 16, 1), dtype=np.uint8)
    neg = (255 - np.tile(tile, (4, 4, 1)))[None]                        # the tiled template's negative: -1 at every multiple of the period
    got = both_kernels(pkg, L, torch_cuda, neg, tile, R.ZNCC)
    assert got.shape == (1, 25, 49) and (got[0, ::8, ::16] == -R.ONE).all() and np.array_equal(got, cpu_match(pkg, L, neg, tile, R.ZNCC))


def test_peak_search_on_the_device(pkg, L, torch_cuda):
    const = np.full((2, 5, 7), 9, np.uint32)
    assert np.array_equal(gpu_peak(pkg, L, torch_cuda, const), [[9, 0, 0, 9, 0, 0]] * 2)
    t = np.zeros((1, 40, 60), np.int32)
    t[0, 10, 44] = t[0, 30, 0] = 77
    t[0, 5, 5] = t[0, 5, 4] = -3
    assert np.array_equal(gpu_peak(pkg, L, torch_cuda, t), [[-3, 4, 5, 77, 44, 10]])
    assert np.array_equal(gpu_peak(pkg, L, torch_cuda, t.view(np.uint32)), [[0, 0, 0, (1 << 32) - 3, 4, 5]])
    rng = np.random.default_rng(91)
    for shape in ((3, 1, 9), (3, 9, 1), (1, 1, 1), (4, 130, 170)):
        for dtype in (np.uint32, np.int32):
            tab = (rng.integers(0, 1 << 32, shape, dtype=np.uint64) >> (28 if shape[-1] == 170 else 0)).astype(np.uint32).view(dtype)      # 16 values: ties
            if dtype == np.int32:
                tab = tab - 7
            want = cpu_peak(pkg, L, tab, 2)
            assert np.array_equal(gpu_peak(pkg, L, torch_cuda, tab), want) and np.array_equal(want, R.peak(tab)), (shape, dtype)
    big = np.zeros((1, 2048, 2050), np.uint32)                          # 4 198 400 entries, the single maximum the last one
    big[0, -1, -1] = 1 << 31
    assert np.array_equal(gpu_peak(pkg, L, torch_cuda, big), [[0, 0, 0, 1 << 31, 2049, 2047]])
    assert pkg.match_peak(big) == [(0, (0, 0), 1 << 31, (2049, 2047))]
