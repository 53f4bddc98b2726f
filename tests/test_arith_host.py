"""The two-image arithmetic without a GPU (mi_blur_arith_value, mi_blur_arith_preset, mi_blur_arith_weighted,
mi_blur_cpu_run_arith, the blocking export on the CPU device, arith() and its wrappers): the definition proved over every
operand pair, exact bytes against arith_ref.py, in-place use, the statuses, the constants arith_ref.py copies, the tiled
kernels' assembly and the sanitizer program."""
import ctypes as C
import itertools
import math
import os

import numpy as np
import pytest

import arith_ref as R
from morph_ref import DILATE, ERODE, ref_morph
from resample_harness import needs_gxx, no_scratch, run_sanitized
from sep_ref import ref_sep, ref_taps

A_ALL, B_ALL = (v.astype(np.int64) for v in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))     # a = row, b = column
OPS = (R.LINEAR, R.ABSDIFF, R.MIN, R.MAX, R.MUL, R.LERP)


def value_table(pkg, L, k, m=0):
    """mi_blur_arith_value over all 65536 (a, b), one call each."""
    ref = C.byref(k)
    call = L.mi_blur_arith_value
    return np.array([[call(ref, a, b, m) for b in range(256)] for a in range(256)], dtype=np.int64)


def cpu_arith(pkg, L, k, a, b, m=None, n_threads=1, guard=64):
    """mi_blur_cpu_run_arith into a buffer of 0xA5 with `guard` bytes either side of the output."""
    a = np.ascontiguousarray(a)
    n, h, w, c = a.shape
    buf = np.full(a.size + 2 * guard, 0xA5, np.uint8)
    pkg.check(L.mi_blur_cpu_run_arith(a.ctypes.data, np.ascontiguousarray(b).ctypes.data, None if m is None else np.ascontiguousarray(m).ctypes.data,
                                      buf.ctypes.data + guard, w, h, c, n, C.byref(k), n_threads), "mi_blur_cpu_run_arith")
    assert (buf[:guard] == 0xA5).all() and (buf[guard + a.size:] == 0xA5).all(), "wrote outside the output"
    return buf[guard:guard + a.size].reshape(a.shape)


def test_presets_are_the_table(pkg, L):
    assert pkg.ARITH_PRESETS == {name: row[0] for name, row in R.PRESETS.items()}
    for name, (pid, *spec) in R.PRESETS.items():
        k = pkg.arith_preset(name)
        assert (k.op, k.wa, k.wb, k.bias, k.shift) == tuple(spec) and (k.b_plane, k.b_shared, k.m_plane, k.m_shared) == (0, 0, 0, 0), name
        assert pkg.arith_preset(pid).op == spec[0]
    k = pkg.Arith()
    assert L.mi_blur_arith_preset(10, C.byref(k)) == pkg.ERR_INVALID and L.mi_blur_arith_preset(-1, C.byref(k)) == pkg.ERR_INVALID
    assert L.mi_blur_arith_preset(0, None) == pkg.ERR_INVALID
    with pytest.raises(ValueError):
        pkg.arith_preset("xor")


@pytest.mark.parametrize("name", sorted(R.PRESETS))
def test_value_of_every_preset_over_all_pairs(pkg, L, name):
    """mi_blur_arith_value == the table's formula for all 65536 (a, b); LERP at five mask values here, every mask below."""
    spec = R.PRESETS[name][1:]
    k = pkg.arith_preset(name)
    for m in ((0, 1, 127, 128, 255) if spec[0] == R.LERP else (0,)):
        got = value_table(pkg, L, k, m)
        assert np.array_equal(got, R.ref_value(spec, A_ALL, B_ALL, m)), (name, m)
        if name == "mul255":
            assert np.array_equal(got, (2 * A_ALL * B_ALL + 255) // 510)
        if name == "lerp" and m in (0, 255):
            assert np.array_equal(got, A_ALL if m == 255 else B_ALL)
    sat = {"add": np.minimum(A_ALL + B_ALL, 255), "sub": np.maximum(A_ALL - B_ALL, 0), "min": np.minimum(A_ALL, B_ALL), "max": np.maximum(A_ALL, B_ALL),
           "absdiff": np.abs(A_ALL - B_ALL), "avg": (A_ALL + B_ALL + 1) // 2, "diff128": np.clip(A_ALL - B_ALL + 128, 0, 255),
           "mulq7": np.minimum((A_ALL * B_ALL + 64) // 128, 255)}
    if name in sat:
        assert np.array_equal(got, sat[name])


def test_lerp_over_all_triples(pkg, L):
    """All 2^24 (a, b, m) as one 4096 x 4096 image through the CPU device, which takes its bytes from the function
    mi_blur_arith_value returns (arith_byte(), filter.h), against the ratio and against both shift forms of the header;
    and the export itself on 20000 random triples."""
    idx = np.arange(1 << 24, dtype=np.int64).reshape(1, 4096, 4096, 1)
    a, b, m = ((idx >> s & 255).astype(np.uint8) for s in (16, 8, 0))
    k = pkg.arith_preset("lerp")
    got = cpu_arith(pkg, L, k, a, b, m, n_threads=0).astype(np.int64)
    t = a.astype(np.int64) * m + b.astype(np.int64) * (255 - m.astype(np.int64))
    want = (2 * t + 255) // 510
    assert np.array_equal(got, want)
    assert np.array_equal(want, (257 * t + 32896) >> 16) and np.array_equal(want, ((t + 128) + ((t + 128) >> 8)) >> 8)
    assert np.array_equal(got[m == 255], a[m == 255]) and np.array_equal(got[m == 0], b[m == 0])
    rng = np.random.default_rng(110)
    for x, y, z in rng.integers(0, 256, size=(20000, 3)):
        assert L.mi_blur_arith_value(C.byref(k), int(x), int(y), int(z)) == (2 * (x * z + y * (255 - z)) + 255) // 510


def test_value_of_random_structs_and_refusals(pkg, L):
    rng = np.random.default_rng(111)
    for op in OPS:
        for _ in range(6):
            spec = R.random_spec(rng, op)
            k = pkg.Arith(*spec)
            pairs = rng.integers(0, 256, size=(400, 3))
            got = [L.mi_blur_arith_value(C.byref(k), int(x), int(y), int(z)) for x, y, z in pairs]
            assert np.array_equal(got, R.ref_value(spec, pairs[:, 0], pairs[:, 1], pairs[:, 2])), spec
    k = pkg.arith_preset("add")
    for bad in ((-1, 0, 0), (256, 0, 0), (0, -1, 0), (0, 256, 0)):
        assert L.mi_blur_arith_value(C.byref(k), *bad) == -1
    assert L.mi_blur_arith_value(C.byref(k), 3, 4, 999) == 7                              # m is ignored unless LERP
    lerp = pkg.arith_preset("lerp")
    assert L.mi_blur_arith_value(C.byref(lerp), 3, 4, 256) == -1 and L.mi_blur_arith_value(C.byref(lerp), 3, 4, -1) == -1
    assert L.mi_blur_arith_value(None, 1, 2, 3) == -1
    for k in invalid_structs(pkg):
        assert L.mi_blur_arith_value(C.byref(k), 1, 2, 3) == -1, fields(k)
    assert pkg.arith_value(pkg.arith_preset("sub"), 9, 4) == 5 and pkg.arith_value(lerp, 10, 20, 255) == 10


def fields(k):
    return tuple(getattr(k, f) for f, _ in k._fields_)


def invalid_structs(pkg):
    """Every row of the validity table, one field wrong at a time."""
    A = pkg.Arith
    W, WM, B = R.MAX_W, R.MAX_W_MUL, R.MAX_BIAS
    rows = [A(6, 0, 0, 0, 0), A(-1, 0, 0, 0, 0),
            A(R.LINEAR, W + 1, 0, 0, 0), A(R.LINEAR, -W - 1, 0, 0, 0), A(R.LINEAR, 0, W + 1, 0, 0), A(R.LINEAR, 0, -W - 1, 0, 0),
            A(R.LINEAR, 1, 1, B + 1, 0), A(R.LINEAR, 1, 1, -B - 1, 0), A(R.LINEAR, 1, 1, 0, 17), A(R.LINEAR, 1, 1, 0, -1),
            A(R.ABSDIFF, 1, 1, 0, 0), A(R.ABSDIFF, W + 1, 0, 0, 0), A(R.ABSDIFF, 1, 0, B + 1, 0), A(R.ABSDIFF, 1, 0, 0, 17),
            A(R.MUL, 1, 1, 0, 0), A(R.MUL, WM + 1, 0, 0, 0), A(R.MUL, -WM - 1, 0, 0, 0), A(R.MUL, 1, 0, -B - 1, 0), A(R.MUL, 1, 0, 0, 17)]
    for op in (R.MIN, R.MAX, R.LERP):
        rows += [A(op, 1, 0, 0, 0), A(op, 0, 1, 0, 0), A(op, 0, 0, 1, 0), A(op, 0, 0, 0, 1)]
    for op in (R.LINEAR, R.ABSDIFF, R.MIN, R.MAX, R.MUL):
        spec = R.PRESETS[{R.LINEAR: "add", R.ABSDIFF: "absdiff", R.MIN: "min", R.MAX: "max", R.MUL: "mulq7"}[op]][1:]
        rows += [A(*spec, 0, 0, 1, 0), A(*spec, 0, 0, 0, 1)]                                # mask flags without LERP
    for flags in ((2, 0, 0, 0), (0, -1, 0, 0), (0, 0, 2, 0), (0, 0, 0, 2)):
        rows.append(A(R.LERP, 0, 0, 0, 0, *flags))
    return rows


def test_limits_are_valid(pkg, L):
    A = pkg.Arith
    W, WM, B = R.MAX_W, R.MAX_W_MUL, R.MAX_BIAS
    for k in (A(R.LINEAR, W, -W, B, 16), A(R.LINEAR, -W, W, -B, 0), A(R.ABSDIFF, -W, 0, B, 16), A(R.MUL, WM, 0, B, 16), A(R.MUL, -WM, 0, -B, 0)):
        spec = fields(k)[:5]
        for a, b in ((255, 255), (0, 255), (255, 0), (0, 0), (1, 254)):
            assert L.mi_blur_arith_value(C.byref(k), a, b, 0) == R.ref_value(spec, a, b), (spec, a, b)


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_cpu_run_random_structs_every_flag(pkg, L, c):
    rng = np.random.default_rng(120 + c)
    for (h, w), n in (((1, 1), 3), ((5, 7), 3), ((64, 96), 2), ((300, 257), 2)):
        shape = (n, h, w, c)
        a = rng.integers(0, 256, size=shape, dtype=np.uint8)
        for op in OPS:
            for bp, bs, mp, ms in itertools.product((0, 1), repeat=4):
                if op != R.LERP and (mp or ms):
                    continue
                if h * w > 10000 and (bp, bs, mp, ms) not in ((0, 0, 0, 0), (1, 1, 0, 0), (0, 1, 1, 0), (1, 0, 0, 1), (1, 1, 1, 1)):
                    continue
                spec = R.random_spec(rng, op) if rng.integers(0, 2) else R.lively_spec(rng, op)
                b = R.operand(rng, shape, bp, bs)
                m = R.operand(rng, shape, mp, ms) if op == R.LERP else None
                k = pkg.Arith(*spec, bp, bs, mp, ms)
                want = R.ref_arith(spec, a, b, m)
                for nt in (1, 4):
                    assert np.array_equal(cpu_arith(pkg, L, k, a, b, m, nt), want), (shape, fields(k), nt)


def test_in_place(pkg, L):
    rng = np.random.default_rng(130)
    shape = (3, 33, 47, 3)
    a0, b0 = (rng.integers(0, 256, size=shape, dtype=np.uint8) for _ in range(2))
    m0 = R.operand(rng, shape, 1, 1)
    plane_b = R.operand(rng, shape, 1, 0)
    n, h, w, c = shape

    def run(k, a, b, m, out, n_images=n):
        return L.mi_blur_cpu_run_arith(a, b, m, out, w, h, c, n_images, C.byref(k), 3)
    for name in ("sub", "absdiff", "mulq7", "lerp"):
        spec = R.PRESETS[name][1:]
        lerp = name == "lerp"
        k = R.struct_of(pkg, spec, b0, m0 if lerp else None, shape)
        want = R.ref_arith(spec, a0, b0, m0 if lerp else None)
        mp = m0.ctypes.data if lerp else None
        a, b = a0.copy(), b0.copy()
        assert run(k, a.ctypes.data, b.ctypes.data, mp, a.ctypes.data) == pkg.OK and np.array_equal(a, want) and np.array_equal(b, b0), name    # out == a
        a = a0.copy()
        assert run(k, a.ctypes.data, b.ctypes.data, mp, b.ctypes.data) == pkg.OK and np.array_equal(b, want) and np.array_equal(a, a0), name    # out == b
        a = a0.copy()
        assert run(k, a.ctypes.data, a.ctypes.data, mp, a.ctypes.data) == pkg.OK                                                                # all three
        assert np.array_equal(a, R.ref_arith(spec, a0, a0, m0 if lerp else None))
    # a shared B may be the output only of a single image; a plane B of a 3-channel image never
    k = pkg.Arith(*R.PRESETS["add"][1:], 0, 1, 0, 0)
    a, b = a0.copy(), b0[:1].copy()
    assert run(k, a.ctypes.data, b.ctypes.data, None, b.ctypes.data) == pkg.ERR_INVALID
    assert run(k, a.ctypes.data, b.ctypes.data, None, b.ctypes.data, 1) == pkg.OK and np.array_equal(b[0], R.ref_arith(k_spec(k), a0[:1], b0[:1])[0])
    k = pkg.Arith(*R.PRESETS["add"][1:], 1, 0, 0, 0)
    big = np.zeros(a0.size, np.uint8)
    assert run(k, a.ctypes.data, big.ctypes.data, None, big.ctypes.data) == pkg.ERR_INVALID
    assert run(k, a.ctypes.data, big.ctypes.data, None, big.ctypes.data, 1) == pkg.ERR_INVALID
    # partial overlaps, and any overlap with the mask
    k = pkg.arith_preset("add")
    room = np.zeros(2 * a0.size + 64, np.uint8)
    base = room.ctypes.data
    for delta in (1, 16, a0.size - 1):
        assert run(k, base + delta, b0.ctypes.data, None, base) == pkg.ERR_INVALID, delta          # out overlaps A from below
        assert run(k, base, b0.ctypes.data, None, base + delta) == pkg.ERR_INVALID, delta          # ... from above
        assert run(k, a0.ctypes.data, base + delta, None, base) == pkg.ERR_INVALID, delta
        assert run(k, a0.ctypes.data, base, None, base + delta) == pkg.ERR_INVALID, delta
    assert run(k, base + a0.size, b0.ctypes.data, None, base) == pkg.OK                            # end to end is no overlap
    lerp = pkg.arith_preset("lerp")
    full_m = np.zeros(a0.size + 8, np.uint8)
    for delta in (0, 1, a0.size - 1):
        assert run(lerp, a0.ctypes.data, b0.ctypes.data, full_m.ctypes.data + delta, full_m.ctypes.data) == pkg.ERR_INVALID, delta    # out == m
    lerp.m_plane = lerp.m_shared = 1
    small = np.zeros(h * w, np.uint8)
    assert run(lerp, a0.ctypes.data, b0.ctypes.data, small.ctypes.data, small.ctypes.data) == pkg.ERR_INVALID
    assert not room[a0.size:].any() and not full_m.any() and not small.any() and not big.any()


def k_spec(k):
    return fields(k)[:5]


def test_statuses(pkg, L):
    OK, INVALID = pkg.OK, pkg.ERR_INVALID
    a, b, m = (np.full((8, 8, 3), v, np.uint8) for v in (10, 20, 30))
    out = np.full((8, 8, 3), 0xA5, np.uint8)
    ia, ib, im, io = a.ctypes.data, b.ctypes.data, m.ctypes.data, out.ctypes.data
    add, lerp = pkg.arith_preset("add"), pkg.arith_preset("lerp")
    no_gpu = L.mi_blur_device_count() <= 0
    calls = {"cpu_run": lambda a_, b_, m_, o_, k, w=8, h=8, c=3, n=1: L.mi_blur_cpu_run_arith(a_, b_, m_, o_, w, h, c, n, k, 1),
             "enqueue": lambda a_, b_, m_, o_, k, w=8, h=8, c=3, n=1: L.mi_blur_enqueue_arith(a_, b_, m_, o_, w, h, c, n, k, None),
             "run_cpu": lambda a_, b_, m_, o_, k, w=8, h=8, c=3, n=1: L.mi_blur_run_arith(pkg.DEVICE_CPU, a_, b_, m_, o_, w, h, c, n, k),
             "run_gpu": lambda a_, b_, m_, o_, k, w=8, h=8, c=3, n=1: L.mi_blur_run_arith(0, a_, b_, m_, o_, w, h, c, n, k)}
    for name, call in calls.items():
        for k in invalid_structs(pkg):
            mask = im if k.op == R.LERP else None
            assert call(ia, ib, mask, io, C.byref(k)) == INVALID, (name, fields(k))
        assert call(ia, ib, None, io, C.byref(lerp)) == INVALID, name                        # LERP without a mask
        assert call(ia, ib, im, io, C.byref(add)) == INVALID, name                           # a mask without LERP
        assert call(None, ib, None, io, C.byref(add)) == INVALID and call(ia, None, None, io, C.byref(add)) == INVALID, name
        assert call(ia, ib, None, None, C.byref(add)) == INVALID and call(ia, ib, None, io, None) == INVALID, name
        for c in (0, 5, -1):
            assert call(ia, ib, None, io, C.byref(add), c=c) == INVALID, (name, c)
        assert call(ia, ib, None, io, C.byref(add), w=0) == INVALID and call(ia, ib, None, io, C.byref(add), h=-1) == INVALID, name
        assert call(ia, ib, None, io, C.byref(add), w=32769, h=1) == INVALID and call(ia, ib, None, io, C.byref(add), w=32768, h=32768) == INVALID, name
        assert call(ia, ib, None, io, C.byref(add), n=-1) == INVALID, name
        assert call(ia, ib, None, io, C.byref(add), n=0) == OK, name
        assert (out == 0xA5).all(), name
        if name in ("enqueue", "run_gpu") and no_gpu:
            assert call(ia, ib, None, io, C.byref(add)) == pkg.ERR_NO_DEVICE and call(ia, ib, im, io, C.byref(lerp)) == pkg.ERR_NO_DEVICE, name
            assert (out == 0xA5).all()
    assert L.mi_blur_run_arith(99, ia, ib, None, io, 8, 8, 3, 1, C.byref(add)) == pkg.ERR_NO_DEVICE
    assert L.mi_blur_run_arith(-2, ia, ib, None, io, 8, 8, 3, 1, C.byref(add)) == pkg.ERR_NO_DEVICE
    assert calls["cpu_run"](ia, ib, None, io, C.byref(add)) == OK and (out == 30).all()
    assert calls["run_cpu"](ia, ib, im, io, C.byref(lerp)) == OK and (out == R.ref_value(R.PRESETS["lerp"][1:], 10, 20, 30)).all()


def test_weighted(pkg, L):
    k = pkg.Arith()
    q = lambda v: math.floor(v * 4096 + 0.5)
    for alpha, beta, gamma in ((0.5, 0.5, 0.0), (1.0, -1.0, 10.0), (16.0, -16.0, 8192.0), (-16.0, 16.0, -8192.0), (0.7, 0.3, -3.25), (1 / 3, 2 / 3, 0.1),
                               (0.5 / 4096, -0.5 / 4096, 0.5 / 4096), (1.5 / 4096, -1.5 / 4096, -0.5 / 4096)):
        assert L.mi_blur_arith_weighted(alpha, beta, gamma, C.byref(k)) == pkg.OK
        assert fields(k) == (R.LINEAR, q(alpha), q(beta), q(gamma) + 2048, 12, 0, 0, 0, 0), (alpha, beta, gamma)
        assert L.mi_blur_arith_value(C.byref(k), 200, 100, 0) == R.ref_value(fields(k)[:5], 200, 100)
    assert (k.wa, k.wb, k.bias) == (2, -1, 2048)                                         # halves round up: floor(x + 0.5)
    assert L.mi_blur_arith_weighted(16.0, -16.0, 8192.0, C.byref(k)) == pkg.OK and (k.wa, k.bias) == (R.MAX_W, (1 << 25) + 2048)
    for bad in ((16.001, 0, 0), (0, -16.001, 0), (0, 0, 8192.5), (0, 0, -8193.0), (math.nan, 0, 0), (0, math.inf, 0), (0, 0, -math.inf)):
        assert L.mi_blur_arith_weighted(*bad, C.byref(k)) == pkg.ERR_INVALID, bad
    assert L.mi_blur_arith_weighted(1.0, 1.0, 0.0, None) == pkg.ERR_INVALID
    # the blend of addWeighted: 0.5 a + 0.5 b rounds half up
    a = np.arange(256, dtype=np.uint8).reshape(16, 16)
    b = a[::-1].copy()
    want = np.clip(np.floor(0.5 * a.astype(np.float64) + 0.5 * b + 0.5), 0, 255).astype(np.uint8)
    assert np.array_equal(pkg.add_weighted(a, 0.5, b, 0.5, device=pkg.DEVICE_CPU), want)
    with pytest.raises(ValueError):
        pkg.add_weighted(a, 17.0, b, 0.5, device=pkg.DEVICE_CPU)


def test_arith_shapes(pkg, L):
    rng = np.random.default_rng(140)
    cpu = pkg.DEVICE_CPU
    n, h, w, c = 4, 9, 11, 3
    a = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    sub, lerp = R.PRESETS["sub"][1:], R.PRESETS["lerp"][1:]
    k, kl = pkg.arith_preset("sub"), pkg.arith_preset("lerp")
    full, shared, plane, shared_plane = (R.operand(rng, a.shape, p, s) for p, s in ((0, 0), (0, 1), (1, 0), (1, 1)))
    for b, given in ((full, full), (shared, shared[0]), (plane, plane), (shared_plane, shared_plane[0]), (shared_plane, shared_plane[0, :, :, 0])):
        for batch in (0, 1, 3):
            assert np.array_equal(pkg.arith(a, given, k, device=cpu, batch=batch), R.ref_arith(sub, a, b)), (given.shape, batch)
            assert np.array_equal(pkg.arith(a, full, kl, mask=given, device=cpu, batch=batch), R.ref_arith(lerp, a, full, b)), (given.shape, batch)
    assert np.array_equal(pkg.arith(a, shared[0], kl, mask=plane, device=cpu, batch=3), R.ref_arith(lerp, a, shared, plane))
    assert np.array_equal(pkg.arith(a, plane, kl, mask=shared[0], device=cpu, batch=3), R.ref_arith(lerp, a, plane, shared))
    assert (k.b_plane, k.b_shared) == (0, 0)                                              # the caller's struct is not written
    # one image, and a grey one
    one = pkg.arith(a[1], full[1], k, device=cpu)
    assert one.shape == (h, w, c) and np.array_equal(one, R.ref_arith(sub, a[1:2], full[1:2])[0])
    assert np.array_equal(pkg.arith(a[1], plane[1], k, device=cpu), R.ref_arith(sub, a[1:2], plane[1:2])[0])
    assert np.array_equal(pkg.arith(a[1], plane[1, :, :, 0], k, device=cpu), R.ref_arith(sub, a[1:2], plane[1:2])[0])
    grey, grey_b = a[0, :, :, 0], a[1, :, :, 1]
    got = pkg.arith(grey, grey_b, k, device=cpu)
    assert got.shape == (h, w) and np.array_equal(got, R.ref_arith(sub, grey[None, :, :, None], grey_b[None, :, :, None])[0, :, :, 0])
    bad = [lambda: pkg.arith(a, full[:3], k, device=cpu), lambda: pkg.arith(a, full[:, :, :, :2], k, device=cpu),
           lambda: pkg.arith(a, full[:, :8], k, device=cpu), lambda: pkg.arith(a, np.zeros((w, h), np.uint8), k, device=cpu),
           lambda: pkg.arith(a, np.zeros((1, h, w, c), np.uint8), k, device=cpu), lambda: pkg.arith(a, full.astype(np.int16), k, device=cpu),
           lambda: pkg.arith(a, np.zeros(h * w, np.uint8), k, device=cpu), lambda: pkg.arith(a, full, k, mask=plane, device=cpu),
           lambda: pkg.arith(a, full, kl, device=cpu), lambda: pkg.arith(a, full, kl, mask=np.zeros((h, w, 2), np.uint8), device=cpu),
           lambda: pkg.arith(np.zeros((2, 4, 4, 5), np.uint8), np.zeros((2, 4, 4, 5), np.uint8), k, device=cpu),
           lambda: pkg.multiply(a, full, "q8", device=cpu), lambda: pkg.blend(a, full, 256, device=cpu),
           lambda: pkg.unsharp_mask(a, 1.0, 16.5, device=cpu), lambda: pkg.running_average(a, full, 0, device=cpu),
           lambda: pkg.running_average(a, full, 9, device=cpu)]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
        assert i >= 0
    with pytest.raises(pkg.MiBlurError):
        pkg.arith(a, full, pkg.Arith(R.LINEAR, 1, 1, 0, 17), device=cpu)


def test_wrappers(pkg, L):
    rng = np.random.default_rng(141)
    cpu = pkg.DEVICE_CPU
    a, b = (rng.integers(0, 256, size=(3, 20, 24, 3), dtype=np.uint8) for _ in range(2))
    x, y = a.astype(np.int64), b.astype(np.int64)
    for got, want in ((pkg.add(a, b, device=cpu), np.minimum(x + y, 255)), (pkg.subtract(a, b, device=cpu), np.maximum(x - y, 0)),
                      (pkg.absdiff(a, b, device=cpu), np.abs(x - y)), (pkg.average(a, b, device=cpu), (x + y + 1) // 2),
                      (pkg.minimum(a, b, device=cpu), np.minimum(x, y)), (pkg.maximum(a, b, device=cpu), np.maximum(x, y)),
                      (pkg.multiply(a, b, device=cpu), (2 * x * y + 255) // 510), (pkg.multiply(a, b, "q7", device=cpu), np.minimum((x * y + 64) >> 7, 255))):
        assert got.dtype == np.uint8 and np.array_equal(got, want)
    mask = rng.integers(0, 256, size=(20, 24), dtype=np.uint8)
    assert np.array_equal(pkg.blend(a, b, mask, device=cpu), R.ref_arith(R.PRESETS["lerp"][1:], a, b, mask[None, :, :, None]))
    assert np.array_equal(pkg.blend(a, b, 255, device=cpu), a) and np.array_equal(pkg.blend(a, b, 0, device=cpu), b)
    assert np.array_equal(pkg.blend(a, b, np.full((20, 24), 255, np.uint8), device=cpu), a)
    assert np.array_equal(pkg.blend(a, b, 128, device=cpu), (2 * (x * 128 + y * 127) + 255) // 510)


def test_compositions(pkg, L):
    rng = np.random.default_rng(142)
    cpu = pkg.DEVICE_CPU
    img = rng.integers(0, 256, size=(2, 40, 48, 3), dtype=np.uint8)
    img[1] = (img[1] // 4 + 90).astype(np.uint8)
    blur = lambda s: ref_sep(img, ref_taps(s), ref_taps(s))
    for sigma, amount in ((1.0, 1.0), (2.5, 0.3), (0.8, 16.0), (1.5, 0.0)):
        g = math.floor(amount * 256 + 0.5)
        want = R.ref_arith((R.LINEAR, 256 + g, -g, 128, 8), img, blur(sigma))
        assert np.array_equal(pkg.unsharp_mask(img, sigma, amount, device=cpu), want), (sigma, amount)
    assert np.array_equal(pkg.unsharp_mask(img, 1.5, 0.0, device=cpu), img)
    assert np.array_equal(pkg.unsharp_mask(img[0, :, :, 0], 1.0, device=cpu),
                          R.ref_arith((R.LINEAR, 512, -256, 128, 8), img[:1, :, :, :1], ref_sep(img[:1, :, :, :1], ref_taps(1.0), ref_taps(1.0)))[0, :, :, 0])
    assert np.array_equal(pkg.difference_of_gaussians(img, 1.0, 2.0, device=cpu, batch=1), R.ref_arith(R.PRESETS["diff128"][1:], blur(1.0), blur(2.0)))
    sub = R.PRESETS["sub"][1:]
    for ksize, (rx, ry) in ((3, (1, 1)), ((5, 3), (2, 1))):
        opened = ref_morph(ref_morph(img, ERODE, rx, ry), DILATE, rx, ry)
        closed = ref_morph(ref_morph(img, DILATE, rx, ry), ERODE, rx, ry)
        assert np.array_equal(pkg.top_hat(img, ksize, device=cpu), R.ref_arith(sub, img, opened)), ksize
        assert np.array_equal(pkg.black_hat(img, ksize, device=cpu), R.ref_arith(sub, closed, img)), ksize
    flat = np.full((30, 30, 3), 77, np.uint8)
    assert not pkg.top_hat(flat, 5, device=cpu).any() and not pkg.black_hat(flat, 5, device=cpu).any()


def test_running_average_converges(pkg, L):
    """A constant frame f.  One step is acc' = acc + floor((f - acc + h) / 2^s) with h = 2^(s-1), so the accumulator stops
    exactly where -h < acc - f <= h, and a distance d above that band shrinks as d' <= d (1 - 2^-s) + 1/2: after
    ceil(ln(d0 - h + 1) / -ln(1 - 2^-s)) + 1 steps the accumulator is in the band and stays.  For shift 1 the band is
    f <= acc <= f + 1: within 1 LSB of the frame, after ceil(log2 d0) + 1 steps.  For larger shifts the definition itself
    (integer accumulator, one rounding) cannot come closer than the band, which is asserted exactly instead."""
    cpu = pkg.DEVICE_CPU
    for shift in (1, 2, 3, 8):
        h = 1 << (shift - 1)
        for start, level in ((0, 200), (255, 13), (100, 101), (7, 7)):
            acc = np.full((8, 8), start, np.uint8)
            frame = np.full((8, 8), level, np.uint8)
            steps = math.ceil(math.log(max(abs(level - start) - h + 1, 1)) / -math.log1p(-2.0 ** -shift)) + 1
            for i in range(steps):
                new = pkg.running_average(acc, frame, shift, device=cpu)
                assert np.array_equal(new, (((1 << shift) - 1) * acc.astype(np.int64) + frame + h) >> shift)
                assert (np.abs(new.astype(int) - level) <= np.abs(acc.astype(int) - level)).all()
                acc = new
            off = acc.astype(int) - level
            assert (-h < off).all() and (off <= h).all(), (shift, start, level, steps)
            assert np.array_equal(pkg.running_average(acc, frame, shift, device=cpu), acc)
            if shift == 1:
                assert (np.abs(off) <= 1).all() and steps == math.ceil(math.log2(max(abs(level - start), 1))) + 1


def test_constants_and_no_scratch(pkg, tmp_path):
    """arith_ref.py's copies of the kernels' units and of the limits, and the tiled kernels compiled to gfx950 assembly (no
    GPU needed): six flat and 24 plane instances, none spills or indexes registers at run time."""
    text = open(os.path.join(pkg.CSRC, "filter.h")).read()
    assert f"constexpr int ARITH_CHUNK = {R.CHUNK};" in text and f"constexpr int ARITH_RUN = {R.RUN};" in text
    assert f"constexpr int ARITH_PLANE_RUN = {R.PLANE_RUN};" in text and f"constexpr int COLOR_GROUP = {R.GROUP};" in text
    assert f"constexpr int ARITH_THREADS = {R.RUN};" in text and R.RUN == R.PLANE_RUN            # one chunk, or one group, per thread
    assert "ARITH_MAX_W = 1 << 16, ARITH_MAX_W_MUL = 1 << 10, ARITH_MAX_BIAS = 1 << 26;" in text and "constexpr int ARITH_MAX_SHIFT = 16;" in text
    header = open(pkg.HEADER).read()
    assert "MI_BLUR_ARITH_LINEAR = 0, MI_BLUR_ARITH_ABSDIFF = 1, MI_BLUR_ARITH_MIN = 2," in header
    assert "MI_BLUR_ARITH_MAX = 3, MI_BLUR_ARITH_MUL = 4, MI_BLUR_ARITH_LERP = 5" in header
    assert (pkg.ARITH_LINEAR, pkg.ARITH_ABSDIFF, pkg.ARITH_MIN, pkg.ARITH_MAX, pkg.ARITH_MUL, pkg.ARITH_LERP) == OPS
    no_scratch(pkg, tmp_path, "arith_kernels.hip", "blur_arith_flat_kernel", 6)
    no_scratch(pkg, tmp_path, "arith_kernels.hip", "blur_arith_plane_kernel", 24)


@needs_gxx
def test_arith_clean_under_asan_ubsan(pkg, tmp_path):
    run_sanitized(pkg, tmp_path, ("san_arith.cpp", "cpu_device.cpp"), ["geometry clean", "arith cases clean", "aliasing clean"])
