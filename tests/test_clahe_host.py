"""CLAHE on the host: mi_blur_clahe_coord and mi_blur_clahe_table against the restatement of clahe_ref.py, the CPU device
against it on shapes whose tiles are one pixel, uneven and whole, the properties the definition promises, every
MI_BLUR_ERR_INVALID case with the output untouched, and the numpy functions on DEVICE_CPU."""
import ctypes as C

import numpy as np
import pytest

from clahe_ref import (BINS, MAX_TILES, ONE, edge, mid, ref_apply, ref_axis, ref_clahe, ref_clipped, ref_coord, ref_table, ref_tables, split_work,
                       tile_box, work_words)
from color_ref import ref_preset
from hist_ref import ref_apply as ref_lookup
from resample_harness import needs_gxx, run_sanitized

CLIPS = (0, 1, 256, 512, 10240, 65536)


def coord(L, S, T, x):
    t0, t1, f = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    assert L.mi_blur_clahe_coord(S, T, x, C.byref(t0), C.byref(t1), C.byref(f)) == 0
    return t0.value, t1.value, f.value


@pytest.mark.parametrize("S,T", [(1, 1), (7, 7), (40, 3), (13, 4), (64, 8), (32768, 64)])
def test_coord_against_the_restatement(pkg, L, S, T):
    a0, a1, af = ref_axis(S, T)
    step = 1 if S <= 64 else 37                                          # ref_coord is a scan over the tiles: not for every x of 32768
    for x in sorted(set(range(0, S, step)) | {S - 1}):
        assert (a0[x], a1[x], af[x]) == ref_coord(S, T, x), x
    for x in range(S):
        t0, t1, f = coord(L, S, T, x)
        assert (t0, t1, f) == (a0[x], a1[x], af[x]), (S, T, x)
        assert 0 <= f < ONE and t1 - t0 in (0, 1) and 0 <= t0 <= t1 < T
        p = 2 * x + 1
        if T == 1 or p <= mid(S, T, 0):
            assert (t0, t1, f) == (0, 0, 0)
        elif p >= mid(S, T, T - 1):
            assert (t0, t1, f) == (T - 1, T - 1, 0)
        else:
            assert t1 == t0 + 1 and mid(S, T, t0) <= p < mid(S, T, t1)
    assert pkg.clahe_coord(S, T, S - 1) == ref_coord(S, T, S - 1)


def table(L, h, A, clip_q8):
    hist = np.asarray(h, dtype=np.uint32)
    lut = np.full(BINS, 0xA5, np.uint8)
    assert L.mi_blur_clahe_table(hist.ctypes.data, A, clip_q8, lut.ctypes.data) == 0
    return lut


def one_bin(v, A):
    h = np.zeros(BINS, np.int64)
    h[v] = A
    return h


def with_residual(residual):
    """A histogram of area 65536 whose excess at clip_q8 = 256 (clip 256) is 256 + residual: one bin of 512 + residual
    over a floor of bins at or below the clip."""
    rest = 65536 - 512 - residual
    h = np.full(BINS, rest // 255, np.int64)
    others = [v for v in range(BINS) if v != 77]
    h[others[:rest % 255]] += 1
    h[77] = 512 + residual
    assert h.sum() == 65536 and max(h[v] for v in others) <= 256 and sum(max(int(x) - 256, 0) for x in h) == 256 + residual
    return h


def test_table_against_python_integers(L):
    rng = np.random.default_rng(2401)
    cases = [(rng.multinomial(5000, rng.dirichlet(np.full(BINS, 0.3))), 5000) for _ in range(6)]
    cases += [(rng.integers(0, 4000, BINS), None), (one_bin(0, 1), 1), (one_bin(255, 1), 1), (one_bin(200, 12345), 12345),
              (one_bin(9, 2**31 - 1), 2**31 - 1)]
    cases += [(with_residual(r), 65536) for r in (0, 1, 128, 255)]
    for h, A in cases:
        A = int(np.asarray(h).sum()) if A is None else A
        for q in CLIPS:
            hp = ref_clipped(h, A, q)
            want = ref_table(h, A, q)
            assert sum(hp) == A and all(a <= b for a, b in zip(want, want[1:])) and want[255] == 255
            assert table(L, h, A, q).tolist() == want, (A, q)
    for r in (0, 1, 128, 255):
        hp = ref_clipped(with_residual(r), 65536, 256)
        assert sum(1 for a, b in zip(hp, with_residual(r)) if a - min(int(b), 256) == 2) == r       # 1 from the quotient, 1 from the residual


def images(rng, n, h, w, c):
    img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    img[0] = (60 + img[0] % 90).astype(np.uint8)                         # a low-contrast image: the clip bites
    return img


def cpu_clahe(pkg, L, img, tiles, clip_q8, mask=0, work=True, threads=3):
    n, h, w, c = img.shape
    k = pkg.Clahe(tiles[0], tiles[1], clip_q8, mask)
    words = work_words(n, tiles, c)
    assert L.mi_blur_clahe_work_bytes(w, h, c, n, C.byref(k)) == 5 * words
    out = np.full_like(img, 0x5A)
    wk = np.full(5 * words + 16, 0x5A, np.uint8) if work else None
    pkg.check(L.mi_blur_cpu_run_clahe(img.ctypes.data, out.ctypes.data, w, h, c, n, C.byref(k), wk.ctypes.data if work else None, threads), "cpu_run_clahe")
    if work:
        assert (wk[5 * words:] == 0x5A).all()
    return out, wk


SHAPES = [(5, 7, (7, 5)), (13, 40, (3, 4)), (48, 64, (8, 8)), (48, 64, (1, 1))]


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_cpu_device_against_the_restatement(pkg, L, c):
    rng = np.random.default_rng(2410 + c)
    for h, w, tiles in SHAPES:
        img = images(rng, 2, h, w, c)
        for mask in (0, 1, 5):
            if mask >> c:
                continue
            for q in (0, 512) if mask else (0, 512, 65536):
                want, want_hist, want_tables = ref_clahe(img, tiles, q, mask)
                out, wk = cpu_clahe(pkg, L, img, tiles, q, mask)
                hist, tables = split_work(wk, 2, tiles, c)
                assert np.array_equal(hist, want_hist) and np.array_equal(tables, want_tables), (h, w, tiles, mask, q)
                assert np.array_equal(out, want), (h, w, tiles, mask, q)
                for j in range(tiles[1]):
                    for i in range(tiles[0]):
                        x0, x1, y0, y1 = tile_box(w, h, *tiles, i, j)
                        assert (hist[:, j, i].sum(axis=-1) == (x1 - x0) * (y1 - y0)).all()
                out2, _ = cpu_clahe(pkg, L, img, tiles, q, mask, work=False)
                assert np.array_equal(out2, want)
                # the two steps on their own
                k = pkg.Clahe(tiles[0], tiles[1], q, mask)
                wk2 = np.zeros_like(wk)
                pkg.check(L.mi_blur_cpu_run_clahe_tables(img.ctypes.data, w, h, c, 2, C.byref(k), wk2.ctypes.data, 2), "cpu_run_clahe_tables")
                assert np.array_equal(wk2[:5 * work_words(2, tiles, c)], wk[:5 * work_words(2, tiles, c)])
                out3 = np.empty_like(img)
                pkg.check(L.mi_blur_cpu_run_clahe_apply(img.ctypes.data, out3.ctypes.data, w, h, c, 2, C.byref(k), tables.ctypes.data, 2), "cpu_run_clahe_apply")
                assert np.array_equal(out3, want)


def test_one_tile_without_a_clip_is_the_global_table(pkg, L):
    img = images(np.random.default_rng(2420), 2, 48, 64, 3)
    out, wk = cpu_clahe(pkg, L, img, (1, 1), 0)
    _, tables = split_work(wk, 2, (1, 1), 3)
    N = 48 * 64
    for i in range(2):
        for ch in range(3):
            cum = np.cumsum(np.bincount(img[i, :, :, ch].reshape(-1), minlength=BINS))
            assert tables[i, 0, 0, ch].tolist() == [(510 * int(cv) + N) // (2 * N) for cv in cum]
    assert np.array_equal(out, ref_lookup(img, tables[:, 0, 0]))


def test_identical_tiles_give_one_table(pkg, L):
    rng = np.random.default_rng(2421)
    tile = (80 + rng.integers(0, 60, size=(12, 16, 2))).astype(np.uint8)
    img = np.tile(tile, (4, 4, 1))[None]
    out, wk = cpu_clahe(pkg, L, np.ascontiguousarray(img), (4, 4), 512)
    _, tables = split_work(wk, 1, (4, 4), 2)
    assert (tables == tables[0, 0, 0]).all() and not np.array_equal(tables[0, 0, 0, 0], np.arange(BINS))
    assert np.array_equal(out, ref_lookup(img, tables[:, 0, 0]))


@pytest.mark.parametrize("c", [1, 3])
def test_apply_with_tables_of_its_callers(pkg, L, c):
    rng = np.random.default_rng(2422 + c)
    n, h, w, tiles = 2, 13, 40, (3, 4)
    img = images(rng, n, h, w, c)
    k = pkg.Clahe(tiles[0], tiles[1], 0, 0)
    one = np.stack([np.stack([rng.permutation(BINS) for _ in range(c)]) for _ in range(n)]).astype(np.uint8)
    same = np.ascontiguousarray(np.broadcast_to(one[:, None, None], (n, tiles[1], tiles[0], c, BINS)))
    per_tile = rng.permuted(np.tile(np.arange(BINS, dtype=np.uint8), (n, tiles[1], tiles[0], c, 1)), axis=-1)
    assert not np.array_equal(per_tile[0, 0, 0], per_tile[0, 0, 1])
    for tables, want in ((same, ref_lookup(img, one)), (per_tile, ref_apply(img, per_tile))):
        out = np.empty_like(img)
        pkg.check(L.mi_blur_cpu_run_clahe_apply(img.ctypes.data, out.ctypes.data, w, h, c, n, C.byref(k), tables.ctypes.data, 2), "cpu_run_clahe_apply")
        assert np.array_equal(out, want)
    assert np.array_equal(ref_apply(img, same), ref_lookup(img, one))


def test_statuses(pkg, L):
    OK, INVALID = pkg.OK, pkg.ERR_INVALID
    a = np.zeros((8, 8, 3), np.uint8)
    b = np.zeros((8, 8, 3), np.uint8)                                   # the output of every call that must fail
    b2 = np.zeros((8, 8, 3), np.uint8)                                  # ... and of the valid ones
    words = work_words(1, (8, 8), 3)                                    # room for the largest grid used here
    work = np.zeros(5 * words + 16, np.uint8)
    tabs = np.zeros(words, np.uint8)
    ia, ib, ib2, iw, it = a.ctypes.data, b.ctypes.data, b2.ctypes.data, work.ctypes.data, tabs.ctypes.data
    assert iw % 16 == 0
    good = pkg.Clahe(2, 2, 512, 0)
    calls = {
        "enqueue_tables": lambda i=ia, o=ib, k=good, wk=iw, w=8, h=8, c=3, n=1: L.mi_blur_enqueue_clahe_tables(i, w, h, c, n, C.byref(k) if k else None, wk, None),
        "enqueue_apply": lambda i=ia, o=ib, k=good, wk=it, w=8, h=8, c=3, n=1: L.mi_blur_enqueue_clahe_apply(i, o, w, h, c, n, C.byref(k) if k else None, wk, None),
        "enqueue": lambda i=ia, o=ib, k=good, wk=iw, w=8, h=8, c=3, n=1: L.mi_blur_enqueue_clahe(i, o, w, h, c, n, C.byref(k) if k else None, wk, None),
        "cpu_tables": lambda i=ia, o=ib, k=good, wk=iw, w=8, h=8, c=3, n=1: L.mi_blur_cpu_run_clahe_tables(i, w, h, c, n, C.byref(k) if k else None, wk, 1),
        "cpu_apply": lambda i=ia, o=ib, k=good, wk=it, w=8, h=8, c=3, n=1: L.mi_blur_cpu_run_clahe_apply(i, o, w, h, c, n, C.byref(k) if k else None, wk, 1),
        "cpu": lambda i=ia, o=ib, k=good, wk=iw, w=8, h=8, c=3, n=1: L.mi_blur_cpu_run_clahe(i, o, w, h, c, n, C.byref(k) if k else None, wk, 1),
        "run_cpu": lambda i=ia, o=ib, k=good, wk=iw, w=8, h=8, c=3, n=1: L.mi_blur_run_clahe(pkg.DEVICE_CPU, i, o, wk, w, h, c, n, C.byref(k) if k else None),
        "run_gpu": lambda i=ia, o=ib, k=good, wk=iw, w=8, h=8, c=3, n=1: L.mi_blur_run_clahe(0, i, o, wk, w, h, c, n, C.byref(k) if k else None),
    }
    has_out = {"enqueue_apply", "enqueue", "cpu_apply", "cpu", "run_cpu", "run_gpu"}
    work_may_be_null = {"cpu", "run_cpu", "run_gpu"}
    bad = [pkg.Clahe(0, 2, 512, 0), pkg.Clahe(2, 0, 512, 0), pkg.Clahe(MAX_TILES + 1, 2, 512, 0), pkg.Clahe(2, MAX_TILES + 1, 512, 0),
           pkg.Clahe(9, 2, 512, 0), pkg.Clahe(2, 9, 512, 0), pkg.Clahe(-1, 2, 512, 0), pkg.Clahe(2, 2, -1, 0), pkg.Clahe(2, 2, 65537, 0),
           pkg.Clahe(2, 2, 512, 8), pkg.Clahe(2, 2, 512, -1)]
    for name, call in calls.items():
        for j, k in enumerate(bad):
            assert call(k=k) == INVALID, (name, j)
        assert call(k=None) == INVALID and call(i=None) == INVALID, name
        if name in work_may_be_null:
            assert call(o=ib2, wk=None) == call(o=ib2) and call(o=ib2) in (OK, pkg.ERR_NO_DEVICE), name
        else:
            assert call(wk=None) == INVALID, name
        if name in has_out:
            assert call(o=None) == INVALID and call(o=ia) == INVALID, name
        for kw in ({"w": 0}, {"h": -1}, {"n": -1}, {"c": 0}, {"c": 5}, {"w": 32769, "h": 2}, {"w": 32768, "h": 32768}):
            assert call(**kw) == INVALID, (name, kw)
        assert call(n=0) == OK, name
        assert call(o=ib2, k=pkg.Clahe(8, 8, 65536, 4)) in (OK, pkg.ERR_NO_DEVICE), name                   # the limits themselves are valid
    for off in (4, 8, 12):
        assert calls["enqueue_tables"](wk=iw + off) == INVALID and calls["enqueue"](wk=iw + off) == INVALID
    for off in (1, 2):
        assert calls["cpu_tables"](wk=iw + off) == INVALID and calls["cpu"](wk=iw + off) == INVALID and calls["run_cpu"](wk=iw + off) == INVALID
        assert calls["run_gpu"](wk=iw + off) == INVALID
    k88 = pkg.Clahe(8, 8, 65536, 7)
    for w, h, c, n in ((0, 8, 3, 1), (8, 8, 0, 1), (8, 8, 5, 1), (8, 8, 3, -1), (32768, 32768, 1, 1)):
        assert L.mi_blur_clahe_work_bytes(w, h, c, n, C.byref(k88)) == 0
    assert L.mi_blur_clahe_work_bytes(8, 8, 3, 1, None) == 0 and L.mi_blur_clahe_work_bytes(7, 8, 3, 1, C.byref(k88)) == 0
    assert L.mi_blur_clahe_work_bytes(8, 8, 3, 2, C.byref(k88)) == 5 * 2 * 64 * 3 * BINS and L.mi_blur_clahe_work_bytes(8, 8, 3, 0, C.byref(k88)) == 0
    assert not b.any(), "an invalid call wrote to the output"
    t0, t1, f = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    for S, T, x in ((0, 1, 0), (32769, 1, 0), (8, 0, 0), (8, 9, 0), (100, MAX_TILES + 1, 0), (8, 2, -1), (8, 2, 8)):
        assert L.mi_blur_clahe_coord(S, T, x, C.byref(t0), C.byref(t1), C.byref(f)) == INVALID, (S, T, x)
    assert L.mi_blur_clahe_coord(8, 2, 0, None, C.byref(t1), C.byref(f)) == INVALID
    assert L.mi_blur_clahe_coord(8, 2, 0, C.byref(t0), None, C.byref(f)) == INVALID
    assert L.mi_blur_clahe_coord(8, 2, 0, C.byref(t0), C.byref(t1), None) == INVALID
    assert (t0.value, t1.value, f.value) == (-7, -7, -7)
    h = np.zeros(BINS, np.uint32)
    h[5] = 10
    lut = np.full(BINS, 0xA5, np.uint8)
    for args in ((None, 10, 512, lut.ctypes.data), (h.ctypes.data, 10, 512, None), (h.ctypes.data, 0, 512, lut.ctypes.data),
                 (h.ctypes.data, 9, 512, lut.ctypes.data), (h.ctypes.data, 11, 512, lut.ctypes.data), (h.ctypes.data, 10, -1, lut.ctypes.data),
                 (h.ctypes.data, 10, 65537, lut.ctypes.data)):
        assert L.mi_blur_clahe_table(*args) == INVALID, args
    assert (lut == 0xA5).all()
    if L.mi_blur_device_count() <= 0:
        for name in ("enqueue_tables", "enqueue_apply", "enqueue", "run_gpu"):
            assert calls[name]() == pkg.ERR_NO_DEVICE, name
            assert calls[name](k=bad[0]) == INVALID and calls[name](i=None) == INVALID, name     # the arguments come first
    assert L.mi_blur_run_clahe(99, ia, ib, None, 8, 8, 3, 1, C.byref(good)) == pkg.ERR_NO_DEVICE
    assert L.mi_blur_version() == 1


def test_numpy_functions_on_the_cpu_device(pkg):
    rng = np.random.default_rng(2430)
    stack = images(rng, 3, 45, 64, 3)
    grey = rng.integers(40, 200, size=(33, 71), dtype=np.uint8)
    cpu = pkg.DEVICE_CPU
    assert np.array_equal(pkg.clahe(stack, device=cpu, batch=2), ref_clahe(stack, (8, 8), 512)[0])
    assert np.array_equal(pkg.clahe(stack, 3.7, (5, 3), channels=(1,), device=cpu), ref_clahe(stack, (5, 3), int(3.7 * 256), 2)[0])
    assert np.array_equal(pkg.clahe(grey, 0, (4, 2), device=cpu), ref_clahe(grey[None, :, :, None], (4, 2), 0)[0][0, :, :, 0])
    assert np.array_equal(pkg.clahe(stack[0], device=cpu), ref_clahe(stack[:1], (8, 8), 512)[0][0])
    luma = ref_preset(ref_clahe(ref_preset(stack, "rgb2ycbcr"), (8, 8), 512, 1)[0], "ycbcr2rgb")
    assert np.array_equal(pkg.clahe(stack, mode="luma", device=cpu, batch=2), luma)
    hist, tables = pkg.clahe_tables(stack, 2.0, (4, 3), device=cpu, batch=2)
    want_hist, want_tables = ref_tables(stack, (4, 3), 512)
    assert np.array_equal(hist, want_hist) and np.array_equal(tables, want_tables)
    h1, t1 = pkg.clahe_tables(grey, 2.0, (4, 3), device=cpu)
    assert h1.shape == (3, 4, 1, BINS) and np.array_equal(t1, ref_tables(grey[None, :, :, None], (4, 3), 512)[1][0])
    assert pkg.clahe_coord(40, 3, 13) == ref_coord(40, 3, 13) and edge(40, 3, 1) == 13
    for bad in (lambda: pkg.clahe(stack, mode="joint", device=cpu), lambda: pkg.clahe(grey, mode="luma", device=cpu),
                lambda: pkg.clahe(stack, -1.0, device=cpu), lambda: pkg.clahe(stack, channels=(3,), device=cpu)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(pkg.MiBlurError):
        pkg.clahe(grey, tiles=(72, 2), device=cpu)


@needs_gxx
def test_clahe_clean_under_asan_ubsan(pkg, tmp_path):
    """A stand-alone program over filter.h and the CPU device: the tiled kernels' geometry walked on the host, the CPU
    device in exact-size buffers, clahe_table() on extreme histograms."""
    run_sanitized(pkg, tmp_path, ("san_clahe.cpp", "cpu_device.cpp"), ["tile geometry clean", "cpu device cases clean", "extreme histograms clean"])
