"""Template matching and the peak search without a GPU: the CPU device (mi_blur_cpu_run_match, mi_blur_cpu_run_match_peak)
and the host export mi_blur_match_value word for word against match_ref.py, the limits of the definition, the Python
functions, the statuses of the nine enqueue / cpu_run / run exports by the rule of test_table_statuses_host.py, the tiled
kernels' scratch size and tests/san_match.cpp under ASan and UBSan."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import match_ref as R
import test_table_statuses_host as T
from resample_harness import needs_gxx, no_scratch, run_sanitized

NAMES = sorted(R.METHODS)


def spec(pkg, method, t, shared):
    return pkg.Match(method, t.shape[-2], t.shape[-3], int(shared))


def cpu_match(pkg, L, img, t, method, n_threads=1):
    """mi_blur_cpu_run_match on (N, H, W, C) and a shared (th, tw, C) or per-image (N, th, tw, C) template, the output
    exactly sized and pre-filled."""
    n, h, w, c = img.shape
    shared = t.ndim == 3
    th, tw = t.shape[-3], t.shape[-2]
    out = np.full((n, h - th + 1, w - tw + 1), 0x5A5A5A5A, np.int32 if method >= R.NCC else np.uint32)
    k = spec(pkg, method, t, shared)
    pkg.check(L.mi_blur_cpu_run_match(img.ctypes.data, np.ascontiguousarray(t).ctypes.data, out.ctypes.data, w, h, c, n, C.byref(k), n_threads),
              "mi_blur_cpu_run_match")
    return out


def cpu_peak(pkg, L, table, n_threads=1):
    n, ho, wo = table.shape
    peaks = np.empty((n, 6), np.int64)
    pkg.check(L.mi_blur_cpu_run_match_peak(table.ctypes.data, int(table.dtype == np.int32), wo, ho, n, peaks.ctypes.data, n_threads),
              "mi_blur_cpu_run_match_peak")
    return peaks


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_cpu_device_equals_the_restatement(pkg, L, c):
    rng = np.random.default_rng(100 + c)
    img = rng.integers(0, 256, (3, 23, 37, c), dtype=np.uint8)
    for tw, th in ((5, 4), (1, 1), (37, 23), (37, 1), (1, 23)):
        for shared in (True, False):
            t = rng.integers(0, 256, (th, tw, c) if shared else (3, th, tw, c), dtype=np.uint8)
            for method in range(5):
                want = R.match(img, t, method)
                for n_threads in (1, 5):
                    got = cpu_match(pkg, L, img, t, method, n_threads)
                    assert got.dtype == want.dtype and np.array_equal(got, want), (tw, th, shared, method, n_threads)


def test_the_extremes(pkg, L):
    img = np.full((1, 129, 130, 4), 255, np.uint8)
    ones = np.full((128, 128, 4), 255, np.uint8)
    zeros = np.zeros((128, 128, 4), np.uint8)
    top = 4261478400
    assert top == 255 * 255 * 65536 and top > 1 << 31
    got = cpu_match(pkg, L, img, ones, R.CCORR)
    assert got.shape == (1, 2, 3) and (got == top).all()
    assert (cpu_match(pkg, L, img, zeros, R.SQDIFF) == top).all()
    assert (cpu_match(pkg, L, img, zeros, R.SAD) == 16711680).all() and 16711680 == 255 * 65536
    assert (cpu_match(pkg, L, img, ones, R.NCC) == R.ONE).all() and (cpu_match(pkg, L, img, ones, R.ZNCC) == 0).all()
    rng = np.random.default_rng(7)
    wide = rng.integers(0, 256, (1, 3, 300, 1), dtype=np.uint8)
    tall = rng.integers(0, 256, (1, 300, 3, 1), dtype=np.uint8)
    for img2, shape in ((wide, (1, 255, 1)), (tall, (255, 1, 1))):
        t = rng.integers(0, 256, shape, dtype=np.uint8)
        for method in range(5):
            assert np.array_equal(cpu_match(pkg, L, img2, t, method, 3), R.match(img2, t, method)), (shape, method)


def test_refused_specs_and_work_bytes(pkg, L):
    img = np.zeros((1, 300, 300, 4), np.uint8)
    out = np.zeros(300 * 300, np.uint32)
    t = np.zeros(1 << 18, np.uint8)

    def status(k, w=300, h=300, c=4, n=1):
        return L.mi_blur_cpu_run_match(img.ctypes.data, t.ctypes.data, out.ctypes.data, w, h, c, n, C.byref(k), 1)

    good = pkg.Match(R.CCORR, 128, 128, 1)
    assert status(good) == pkg.OK and L.mi_blur_match_work_bytes(300, 300, 4, 1, C.byref(good)) > 0
    bad = [pkg.Match(R.CCORR, 256, 1, 1), pkg.Match(R.CCORR, 1, 256, 1), pkg.Match(R.CCORR, 0, 1, 1), pkg.Match(R.CCORR, 1, 0, 1),
           pkg.Match(5, 3, 3, 1), pkg.Match(-1, 3, 3, 1), pkg.Match(R.CCORR, 3, 3, 2), pkg.Match(R.CCORR, 3, 3, -1)]
    assert 129 * 127 * 4 <= R.MAX_AREA and status(pkg.Match(R.CCORR, 129, 127, 1)) == pkg.OK
    for k in bad:
        assert status(k) == pkg.ERR_INVALID, (k.method, k.tw, k.th, k.t_shared)
        assert L.mi_blur_match_work_bytes(300, 300, 4, 1, C.byref(k)) == 0
    k = pkg.Match(R.CCORR, 65537, 1, 1)                                 # tw * th * C = 65 537 needs C = 1 and a side over 255 ...
    assert status(k, 70000, 1, 1) == pkg.ERR_INVALID
    k = pkg.Match(R.CCORR, 241, 68, 1)                                  # ... or four channels: 241 * 68 * 4 = 65 552 > 65 536
    assert status(k) == pkg.ERR_INVALID and L.mi_blur_match_work_bytes(300, 300, 4, 1, C.byref(k)) == 0
    k = pkg.Match(R.CCORR, 9, 3, 1)                                     # wider than the image
    assert status(k, 8, 8, 3) == pkg.ERR_INVALID
    assert L.mi_blur_match_work_bytes(300, 300, 4, 1, None) == 0 and L.mi_blur_match_work_bytes(300, 300, 5, 1, C.byref(good)) == 0
    assert L.mi_blur_match_work_bytes(0, 300, 4, 1, C.byref(good)) == 0 and L.mi_blur_match_work_bytes(300, 300, 4, -1, C.byref(good)) == 0
    assert L.mi_blur_match_peak_work_bytes(0, 4, 1) == 0 and L.mi_blur_match_peak_work_bytes(4, 0, 1) == 0
    assert L.mi_blur_match_peak_work_bytes(4, 4, -1) == 0 and L.mi_blur_match_peak_work_bytes(1 << 16, 1 << 16, 1) == 0
    assert L.mi_blur_match_peak_work_bytes(4, 4, 2) == 2 * pkg.MATCH_PEAK_PARTS * 16
    with pytest.raises(ValueError):
        pkg.match_template(img[0], np.zeros((1, 256, 4), np.uint8), "ccorr", pkg.DEVICE_CPU)
    with pytest.raises(ValueError):
        pkg.match_template(img[0], np.zeros((68, 241, 4), np.uint8), "ccorr", pkg.DEVICE_CPU)


def two_level(rng, A):
    """Sums of a window and a template of A bytes that exist: each is one byte value on a prefix and another on the rest."""
    na, nt = int(rng.integers(0, A + 1)), int(rng.integers(0, A + 1))
    a1, a2, t1, t2 = (int(v) for v in rng.integers(0, 256, 4))
    if rng.integers(0, 4) == 0:
        t1, t2 = a1, a2                                                 # proportional or equal operands: the scores near one
        nt = na if rng.integers(0, 2) else nt
    lo, hi = min(na, nt), max(na, nt)
    mid = (a1 * t2 if na > nt else a2 * t1) * (hi - lo)
    sum_at = a1 * t1 * lo + mid + a2 * t2 * (A - hi)
    return (sum_at, a1 * na + a2 * (A - na), a1 * a1 * na + a2 * a2 * (A - na), t1 * nt + t2 * (A - nt), t1 * t1 * nt + t2 * t2 * (A - nt))


def test_match_value_equals_python_integers(pkg, L):
    rng = np.random.default_rng(11)
    for i in range(100000):
        A = int(rng.integers(1, 65537)) if i % 2 else int(rng.integers(1, 65))
        sums = two_level(rng, A)
        method = R.NCC + (i >> 1) % 2
        want = R.value(method, A, *sums)
        assert want is not None and L.mi_blur_match_value(method, A, *sums) == want, (method, A, sums)


def test_match_value_adversarial(pkg, L):
    value = lambda *a: L.mi_blur_match_value(*a)
    NONE = -(1 << 31)
    # N^2 = D exactly: +-16384.
    assert value(R.NCC, 4, 1000, 60, 1000, 60, 1000) == R.ONE
    a, t = [10, 20, 30, 250], [250, 240, 230, 10]                       # t = 260 - a: ZNCC is exactly -1
    sums = (sum(x * y for x, y in zip(a, t)), sum(a), sum(x * x for x in a), sum(t), sum(x * x for x in t))
    assert value(R.ZNCC, 4, *sums) == -R.ONE == R.value(R.ZNCC, 4, *sums)
    assert value(R.ZNCC, 4, sums[2], sums[1], sums[2], sums[1], sums[2]) == R.ONE
    # Exactly on a half: NCC with sum_aa = sum_tt = 2^15 m, so sqrt(D) = 2^15 m and 2^14 N / sqrt(D) = N / (2m); N = (2k - 1) m
    # is k - 1/2, which rounds away from zero to k; one unit of N below it stays at k - 1 (m > 1) or lands on k - 1 exactly.
    for m in (1, 3, 127):
        s = (1 << 15) * m
        A = 65536
        for k in (1, 2, 3, 100, 8191, 8192, 16383, 16384):
            N = (2 * k - 1) * m
            for n_at in (N - 1, N, N + 1):
                if not 0 <= n_at <= s:
                    continue
                want = R.value(R.NCC, A, n_at, 0, s, 0, s)
                assert value(R.NCC, A, n_at, 0, s, 0, s) == want, (m, k, n_at)
                if n_at == N:
                    assert want == k
                if n_at == N - 1:
                    assert want == k - 1
    # The same for ZNCC: sum_a = sum_t = 0 leaves N = A sum_at and D = (A s)^2.
    for k in (1, 5000, 16384):
        s, N = 1 << 15, 2 * k - 1
        for n_at in (N - 1, N, N + 1):
            if n_at <= s:
                assert value(R.ZNCC, 16, n_at, 0, s, 0, s) == R.value(R.ZNCC, 16, n_at, 0, s, 0, s) == (k - 1 if n_at < N else k)
    # D = 0, N = 0, N < 0.
    assert value(R.NCC, 9, 0, 0, 0, 90, 900) == 0 and value(R.ZNCC, 9, 900, 90, 900, 90, 900) == 0
    assert value(R.ZNCC, 4, 0, 0, 0, 0, 0) == 0 and value(R.NCC, 4, 0, 10, 100, 10, 100) == 0
    assert value(R.ZNCC, 2, 0, 10, 100, 10, 100) == -R.ONE == R.value(R.ZNCC, 2, 0, 10, 100, 10, 100)
    assert value(R.ZNCC, 4, 25, 10, 50, 10, 50) == 0 == R.value(R.ZNCC, 4, 25, 10, 50, 10, 50)     # N = 0 with D > 0
    # Every refusal.
    good = (R.NCC, 4, 1000, 60, 1000, 60, 1000)
    assert value(*good) != NONE
    for bad in ((R.CCORR,) + good[1:], (5,) + good[1:], (R.NCC, 0) + good[2:], (R.NCC, 65537) + good[2:],
                (R.NCC, 4, 1000, 1021, 1 << 20, 60, 1000),             # sum_a > 255 A
                (R.NCC, 4, 1000, 60, 65025 * 4 + 1, 60, 1000),         # sum_aa > 65025 A
                (R.NCC, 4, 1000, 64, 1000, 60, 1000),                  # sum_a^2 > A sum_aa
                (R.NCC, 4, 1000, 60, 1000, 1021, 1 << 20), (R.NCC, 4, 1000, 60, 1000, 60, 65025 * 4 + 1), (R.NCC, 4, 1000, 60, 1000, 64, 1000),
                (R.NCC, 4, 1001, 60, 1000, 60, 1000)):                 # sum_at^2 > sum_aa sum_tt
        assert value(*bad) == NONE and R.value(*bad) is None, bad
    assert pkg.match_value("ncc", *good[1:]) == R.ONE and pkg.match_value("zncc", 0, 0, 0, 0, 0, 0) is None
    assert pkg.match_value("ncc", 4, 1 << 32, 0, 0, 0, 0) is None


def test_a_planted_patch(pkg, L):
    rng = np.random.default_rng(21)
    img = rng.integers(0, 256, (40, 52, 3), dtype=np.uint8)
    x, y = 17, 9
    t = img[y:y + 7, x:x + 11].copy()
    for name in ("sqdiff", "sad"):
        table = pkg.match_template(img, t, name, pkg.DEVICE_CPU)
        assert table.dtype == np.uint32 and table.shape == (34, 42) and table[y, x] == 0 and np.count_nonzero(table == 0) == 1
    assert pkg.match_template(img, t, "zncc", pkg.DEVICE_CPU)[y, x] == R.ONE == pkg.match_template(img, t, "ncc", pkg.DEVICE_CPU)[y, x]
    for name in NAMES:
        pos, value = pkg.find_template(img, t, name, pkg.DEVICE_CPU)
        assert pos == (x, y), name
        assert value == int(pkg.match_template(img, t, name, pkg.DEVICE_CPU)[y, x])
    # A stack with per-image templates, and grey images without a channel axis.
    stack = rng.integers(0, 256, (2, 30, 30, 1), dtype=np.uint8)
    ts = np.stack([stack[0, 3:8, 4:10], stack[1, 20:25, 11:17]])
    assert [p for p, _ in pkg.find_template(stack, ts, "sad", pkg.DEVICE_CPU)] == [(4, 3), (11, 20)]
    grey = stack[0, :, :, 0]
    assert pkg.find_template(grey, grey[3:8, 4:10], "zncc", pkg.DEVICE_CPU) == ((4, 3), R.ONE)
    assert np.array_equal(pkg.match_template(stack, ts, "ccorr", pkg.DEVICE_CPU), R.match(stack, ts, R.CCORR))


def test_peak_search(pkg, L):
    const = np.full((2, 5, 7), 9, np.uint32)
    assert np.array_equal(cpu_peak(pkg, L, const), [[9, 0, 0, 9, 0, 0]] * 2)
    t = np.zeros((1, 4, 6), np.uint32)
    t[0, 1, 4] = t[0, 3, 0] = 77                                        # two equal maxima: the earlier one; the minimum ties at (0, 0)
    assert np.array_equal(cpu_peak(pkg, L, t), [[0, 0, 0, 77, 4, 1]])
    t = np.full((1, 4, 6), 50, np.uint32)
    t[0, 2, 5] = t[0, 3, 1] = 3                                         # two equal minima
    assert np.array_equal(cpu_peak(pkg, L, t), [[3, 5, 2, 50, 0, 0]])
    s = np.array([[[5, -7, 3], [-7, 100, -(1 << 31)], [(1 << 31) - 1, 0, (1 << 31) - 1]]], np.int32)
    assert np.array_equal(cpu_peak(pkg, L, s), [[-(1 << 31), 2, 1, (1 << 31) - 1, 0, 2]])
    u = s.view(np.uint32)                                               # the same words unsigned: entries >= 2^31
    assert np.array_equal(cpu_peak(pkg, L, u), [[0, 1, 2, (1 << 32) - 7, 1, 0]])
    rng = np.random.default_rng(3)
    for shape in ((3, 1, 9), (3, 9, 1), (1, 1, 1), (4, 13, 17)):
        for dtype in (np.uint32, np.int32):
            t = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32).view(dtype)
            t[..., 0] = t[..., -1]                                      # ties
            for n_threads in (1, 5):
                assert np.array_equal(cpu_peak(pkg, L, t, n_threads), R.peak(t)), (shape, dtype)
    assert pkg.match_peak(s[0], pkg.DEVICE_CPU) == (-(1 << 31), (2, 1), (1 << 31) - 1, (0, 2))
    assert pkg.match_peak(u, pkg.DEVICE_CPU) == [(0, (1, 2), (1 << 32) - 7, (1, 0))]
    peaks = np.empty(6, np.int64)
    for bad in ((None, 0, 3, 3, 1, peaks.ctypes.data), (s.ctypes.data, 2, 3, 3, 1, peaks.ctypes.data), (s.ctypes.data, 0, 0, 3, 1, peaks.ctypes.data),
                (s.ctypes.data, 0, 3, 3, -1, peaks.ctypes.data), (s.ctypes.data, 0, 3, 3, 1, None), (s.ctypes.data + 1, 0, 2, 2, 1, peaks.ctypes.data),
                (s.ctypes.data, 0, 3, 3, 1, peaks.ctypes.data + 4)):
        assert L.mi_blur_cpu_run_match_peak(*bad, 1) == pkg.ERR_INVALID


# ---------------------------------------------------------------- statuses, by the rule of test_table_statuses_host.py
E = T.Export
_p = T._p
# The pointers of that table: "i" the images, "b" the template, "o" the output (the peaks), "t" the table, "wk" the work
# buffer.  The peak search has no channel count: its `channels` column carries is_signed (channels - 3: 0, and 2 for the
# "channels 5" case, which is as invalid there).
EXPORTS = {
    "mi_blur_enqueue_match": E("enqueue", "match",
                               lambda L, a: L.mi_blur_enqueue_match(a["i"], a["b"], a["o"], a["w"], a["h"], a["c"], a["n"], _p(a["k"]), a["wk"], None),
                               ("i", "b", "o", "wk"), {"o": 16, "wk": 16}, {"out == in": dict(o="i"), "out == template": dict(o="b")}),
    "mi_blur_cpu_run_match": E("cpu_run", "match",
                               lambda L, a: L.mi_blur_cpu_run_match(a["i"], a["b"], a["o"], a["w"], a["h"], a["c"], a["n"], _p(a["k"]), 1),
                               ("i", "b", "o"), {"o": 4}, {"out == in": dict(o="i"), "out == template": dict(o="b")}),
    "mi_blur_run_match": E("run", "match",
                           lambda L, a: L.mi_blur_run_match(a["dev"], a["i"], a["b"], a["o"], a["w"], a["h"], a["c"], a["n"], _p(a["k"])),
                           ("i", "b", "o"), {"o": 4}, {"out == in": dict(o="i"), "out == template": dict(o="b")}, cpu="mi_blur_cpu_run_match"),
    "mi_blur_enqueue_match_peak": E("enqueue", None,
                                    lambda L, a: L.mi_blur_enqueue_match_peak(a["t"], a["c"] - T.CH, a["w"], a["h"], a["n"], a["o"], a["wk"], None),
                                    ("t", "o", "wk"), {"t": 16, "o": 16, "wk": 16}),
    "mi_blur_cpu_run_match_peak": E("cpu_run", None,
                                    lambda L, a: L.mi_blur_cpu_run_match_peak(a["t"], a["c"] - T.CH, a["w"], a["h"], a["n"], a["o"], 1),
                                    ("t", "o"), {"t": 4, "o": 8}),
    "mi_blur_run_match_peak": E("run", None,
                                lambda L, a: L.mi_blur_run_match_peak(a["dev"], a["t"], a["c"] - T.CH, a["w"], a["h"], a["n"], a["o"]),
                                ("t", "o"), {"t": 4, "o": 8}, cpu="mi_blur_cpu_run_match_peak"),
}


def _structs(pkg):
    k = pkg.Match(pkg.MATCH_ZNCC, 3, 3, 1)
    return {"match": (k, T._edit(k, tw=T.W + 1))}


@pytest.fixture()
def table(monkeypatch):
    """test_table_statuses_host's statuses() and expected() over the exports above."""
    monkeypatch.setattr(T, "EXPORTS", EXPORTS)
    monkeypatch.setattr(T, "_structs", _structs)
    return T


def _work_fits(pkg, L):
    sizes = [L.mi_blur_match_work_bytes(T.W, T.H, T.CH, 1, C.byref(pkg.Match(m, 3, 3, 1))) for m in range(5)]
    sizes.append(L.mi_blur_match_peak_work_bytes(T.W, T.H, 1))
    return all(0 < b <= T.BUF for b in sizes)


def test_the_table_names_every_match_export(pkg):
    mine = re.compile(r"mi_blur_(enqueue|cpu_run|run)_match\w*")
    assert sorted(s for s in pkg.declared_symbols() if mine.fullmatch(s)) == sorted(EXPORTS)


def test_statuses_without_a_device(pkg, L, table):
    if L.mi_blur_device_count() > 0:
        pytest.skip("the column of a machine without a GPU")
    assert _work_fits(pkg, L)
    host, keep = table._host_buffers()
    got = table.statuses(pkg, L, host, host)
    table._assert_table(got, table.expected(got, False))
    for name, cases in (("mi_blur_enqueue_match", ("null i", "null b", "null o", "null wk", "o + 1", "o + 4", "wk + 1", "wk + 4", "width 0", "channels 5",
                                                   "n_images -1", "invalid struct", "null struct", "out == in", "out == template", "good",
                                                   "good, n_images 0")),
                        ("mi_blur_run_match_peak", ("null t", "t + 1", "o + 1", "channels 5", "good on ordinal 99", "good, n_images 0 on ordinal -2"))):
        assert all(c in got[name] for c in cases), name
    assert keep


def test_run_on_the_cpu_device_gives_the_bytes_of_cpu_run(pkg, L):
    assert _work_fits(pkg, L)
    k = _structs(pkg)["match"][0]
    for name, e in EXPORTS.items():
        if e.kind != "run":
            continue
        left = []
        for export in (e, EXPORTS[e.cpu]):
            addr, arrays = T._host_buffers(np.random.default_rng(5))
            arrays["o"][:] = 0xA5
            a = dict(addr, w=T.W, h=T.H, c=T.CH, n=1, k=k, dev=pkg.DEVICE_CPU)
            assert export.call(L, a) == T.OK, name
            left.append(arrays["o"].copy())
        assert np.array_equal(left[0], left[1]) and (left[0] != 0xA5).any(), name


@pytest.mark.gpu
def test_statuses_with_a_device(pkg, L, table):
    import torch
    assert torch.cuda.is_available() and L.mi_blur_device_count() >= 1
    assert _work_fits(pkg, L)
    tensors = {p: torch.zeros(T.BUF, dtype=torch.uint8, device="cuda") for p in T.POINTERS}
    host, keep = table._host_buffers()
    got = table.statuses(pkg, L, {p: t.data_ptr() for p, t in tensors.items()}, host)
    torch.cuda.synchronize()
    table._assert_table(got, table.expected(got, True))
    assert keep


# ---------------------------------------------------------------- the code objects and the sanitizers
def test_tiled_match_kernels_use_no_scratch(pkg, tmp_path):
    """Compiles match_kernels.hip to gfx950 assembly (no GPU needed): the three tiled instantiations (SQDIFF, CCORR, SAD)
    keep their accumulators and aligned dwords in registers; all their LDS is sized per launch."""
    no_scratch(pkg, tmp_path, "match_kernels.hip", "blur_match_tiled_kernel", 3, dynamic_lds_only=True)
    text = open(os.path.join(pkg.CSRC, "filter.h")).read()
    assert "MATCH_TX = 64, MATCH_R = 4, MATCH_TY = MATCH_THREADS / 64 * MATCH_R" in text and R.TILE == (64, 16)     # match_ref.py's copy


def test_the_other_match_kernels_use_no_scratch(pkg, tmp_path):
    no_scratch(pkg, tmp_path, "match_kernels.hip", "blur_match_(?:prep|generic|score|peak|peak_final)_kernel", 5)


@needs_gxx
def test_match_clean_under_asan_ubsan(pkg, tmp_path):
    run_sanitized(pkg, tmp_path, ("san_match.cpp", "cpu_device.cpp"), ["match cases clean", "peak cases clean", "score cases clean"])
