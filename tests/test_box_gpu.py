"""The integral images and the box filters on the GPU (mi_blur_enqueue_integral, mi_blur_enqueue_box_from_integral,
mi_blur_enqueue_box, integral() and its kin on device 0): exact tables and exact bytes against box_ref.py and the CPU
device, inside guard patterns, and which kernel took each launch."""
import ctypes as C

import numpy as np
import pytest

import box_ref as R
from resample_harness import last, torch_cuda  # noqa: F401
from table_harness import Guarded, stream, upload

pytestmark = pytest.mark.gpu

ONES = 0xFFFFFFFF
B = R.BAND
GUARD = 16                                    # words in front of a table (64 bytes: the table stays 16-byte aligned) and behind it
RADII = [(0, 0), (1, 1), (1, 7), (16, 16), (127, 0), (0, 127), (127, 127)]
OPS = (R.MEAN, R.STDDEV, R.THRESHOLD)
# (W, H): every width and every height of the kernel's units occurs
UNITS = [(16, 1), (16, 2 * B + 1), (1008, B - 1), (1024, B), (1040, B + 1), (1024, 2 * B + 1), (R.MAX_W, 1), (R.MAX_W, 2 * B + 1),
         (R.MAX_W + 16, B + 1)]


def spec(pkg, op, rx, ry):
    return pkg.Box(op, rx, ry, -3, rx & 1) if op == R.THRESHOLD else pkg.Box(op, rx, ry, 0, 0)


def device_tables(pkg, L, torch, ptr, shape, want_s=True, want_q=True):
    """mi_blur_enqueue_integral on the images at ptr: every table inside 0xFFFFFFFF words, the work buffer inside 0x5A bytes.
    Returns (S, Q, work as uint32, the device buffers of S and Q): None where not asked."""
    n, h, w, c = shape
    words = n * h * w * c
    bufs = [Guarded(torch, words, "the table", np.uint32, ONES, GUARD, GUARD) if on else None for on in (want_s, want_q)]
    ptrs = [None if b is None else b.ptr for b in bufs]
    nwork = L.mi_blur_integral_work_bytes(w, h, c, n, int(want_s and want_q))
    assert nwork == R.work_bytes(shape, 2 if want_s and want_q else 1)
    d_work = Guarded(torch, nwork, "the work buffer")
    assert all(p is None or p % 16 == 0 for p in ptrs)
    pkg.check(L.mi_blur_enqueue_integral(ptr, ptrs[0], ptrs[1], w, h, c, n, d_work.ptr, stream(torch)), "mi_blur_enqueue_integral")
    torch.cuda.synchronize()
    out = [None if b is None else b.payload().reshape(shape) for b in bufs]
    return out[0], out[1], d_work.payload().view(np.uint32), bufs


def cpu_tables(pkg, L, img):
    S, Q = np.empty(img.shape, np.uint32), np.empty(img.shape, np.uint32)
    n, h, w, c = img.shape
    pkg.check(L.mi_blur_cpu_run_integral(img.ctypes.data, S.ctypes.data, Q.ctypes.data, w, h, c, n, 4), "mi_blur_cpu_run_integral")
    return S, Q


def check_integral(pkg, L, torch, img, kernel, offset_in=0, work_too=False):
    """One launch for S and Q together, then each alone: all equal box_ref.py and the CPU device, in `kernel`."""
    d, ptr = upload(torch, img, offset_in)
    wantS, wantQ = R.ref_integral(img), R.ref_integral(img, True)
    cS, cQ = cpu_tables(pkg, L, img)
    assert np.array_equal(cS, wantS) and np.array_equal(cQ, wantQ)
    S, Q, work, _ = device_tables(pkg, L, torch, ptr, img.shape)
    assert last(L) == kernel
    assert np.array_equal(S, wantS) and np.array_equal(Q, wantQ), img.shape
    if work_too:                                   # work[image][band][S, Q][W * C]: the column sums of the rows above the band
        n, h, w, c = img.shape
        nb = -(-h // B)
        col = [np.cumsum(v, axis=1, dtype=np.uint64) for v in (img.astype(np.uint64), img.astype(np.uint64) ** 2)]
        want = np.zeros((n, nb, 2, w * c), np.uint32)
        for b in range(1, nb):
            for t in range(2):
                want[:, b, t] = (col[t][:, b * B - 1].reshape(n, w * c) % R.M32).astype(np.uint32)
        assert np.array_equal(work.reshape(n, nb, 2, w * c), want)
    S1, none, _, _ = device_tables(pkg, L, torch, ptr, img.shape, True, False)
    assert last(L) == kernel and none is None and np.array_equal(S1, wantS)
    none, Q1, _, _ = device_tables(pkg, L, torch, ptr, img.shape, False, True)
    assert last(L) == kernel and none is None and np.array_equal(Q1, wantQ)


def device_box(pkg, L, torch, p_in, tabs, shape, k, offset_out=0, in_place=False):
    """mi_blur_enqueue_box_from_integral from the device tables `tabs` (S, Q): the output lies offset_out bytes into a buffer of
    0x5A with 128 bytes to spare, or is the input itself."""
    n, h, w, c = shape
    size = n * h * w * c
    d_out = Guarded(torch, size, "the output", front=offset_out, back=128 - offset_out)
    p_out = p_in if in_place else d_out.ptr
    pS, pQ = (t.ptr for t in tabs)
    pkg.check(L.mi_blur_enqueue_box_from_integral(p_in if k.op == R.THRESHOLD else None, pS, pQ if k.op == R.STDDEV else None, p_out, w, h, c, n,
                                                  C.byref(k), stream(torch)), "mi_blur_enqueue_box_from_integral")
    torch.cuda.synchronize()
    if in_place:
        return None
    return d_out.payload().reshape(shape)


def cpu_box(pkg, L, img, k):
    out = np.empty_like(img)
    n, h, w, c = img.shape
    pkg.check(L.mi_blur_cpu_run_box(img.ctypes.data, out.ctypes.data, w, h, c, n, C.byref(k), 4), "mi_blur_cpu_run_box")
    return out


def two_images(rng, h, w, c):
    img = rng.integers(0, 256, size=(2, h, w, c), dtype=np.uint8)
    img[1, :, w // 2:] = (img[1, :, w // 2:] // 8 + 90).astype(np.uint8)          # the second image differs, and is flat in one half
    return img


# ---------------------------------------------------------------- the integral
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_integral_at_the_kernels_units(pkg, L, torch_cuda, c):
    rng = np.random.default_rng(200 + c)
    assert {w for w, _ in UNITS} == {16, R.WAVE_SPAN - 16, R.WAVE_SPAN, R.WAVE_SPAN + 16, R.MAX_W, R.MAX_W + 16}
    assert {h for _, h in UNITS} == {1, B - 1, B, B + 1, 2 * B + 1}
    for w, h in UNITS:
        img = two_images(rng, h, w, c)
        tiled = R.integral_takes_tiled(img.shape)
        assert tiled == (w <= R.MAX_W)
        check_integral(pkg, L, torch_cuda, img, R.INTEGRAL_TILED if tiled else R.INTEGRAL_GENERIC, work_too=tiled)


def test_integral_other_launches_take_the_generic_kernel(pkg, L, torch_cuda):
    rng = np.random.default_rng(205)
    for h, w in ((5, 17), (1, 1), (B + 3, 65), (3, 130)):
        for c in (1, 2, 3, 4):
            img = two_images(rng, h, w, c)
            assert not R.integral_takes_tiled(img.shape)
            check_integral(pkg, L, torch_cuda, img, R.INTEGRAL_GENERIC)
    img = two_images(rng, B + 2, 48, 3)
    check_integral(pkg, L, torch_cuda, img, R.INTEGRAL_TILED)
    for off in (1, 8):                                                            # an input pointer off 16 bytes
        assert not R.integral_takes_tiled(img.shape, off)
        check_integral(pkg, L, torch_cuda, img, R.INTEGRAL_GENERIC, off)


def test_integral_wraps_and_the_windows_stay_exact(pkg, L, torch_cuda):
    """An all-255 image of 4112 x 4097: the table passes 2^32 in its last rows; the tiled kernel, and the fused box mean."""
    torch = torch_cuda
    h, w = 4097, 4112
    assert h * w * 255 > R.M32 and R.integral_takes_tiled((1, h, w, 1))
    d_in = torch.full((h * w,), 255, dtype=torch.uint8, device="cuda")
    S, _, _, _ = device_tables(pkg, L, torch, d_in.data_ptr(), (1, h, w, 1), True, False)
    assert last(L) == R.INTEGRAL_TILED
    rows, cols = np.arange(1, h + 1, dtype=np.uint64)[:, None], np.arange(1, w + 1, dtype=np.uint64)[None, :]
    want = ((rows * cols * np.uint64(255)) % np.uint64(R.M32)).astype(np.uint32)
    assert np.array_equal(S[0, :, :, 0], want)
    assert (np.diff(S[0, -1, :, 0].astype(np.int64)) < 0).any(), "the last row never wrapped"
    k = pkg.Box(R.MEAN, 127, 15, 0, 0)
    nwork = L.mi_blur_box_work_bytes(w, h, 1, 1, C.byref(k))
    d_work = torch.full((nwork + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    d_out = torch.full((h * w + 128,), 0x5A, dtype=torch.uint8, device="cuda")
    pkg.check(L.mi_blur_enqueue_box(d_in.data_ptr(), d_out.data_ptr(), w, h, 1, 1, C.byref(k), d_work.data_ptr(), stream(torch)), "mi_blur_enqueue_box")
    torch.cuda.synchronize()
    assert last(L) == R.BOX_TILED
    assert bool((d_out[:h * w] == 255).all()) and bool((d_out[h * w:] == 0x5A).all()) and bool((d_work[nwork:] == 0x5A).all())


def test_integral_with_other_bands(pkg, L, torch_cuda):
    """The A/B knob: bands of 8 and of 64 rows give the same tables."""
    rng = np.random.default_rng(206)
    img = two_images(rng, 70, 1040, 3)
    d, ptr = upload(torch_cuda, img)
    n, h, w, c = img.shape
    try:
        for band in (8, 64, 1):
            assert L.mi_blur_set_option(b"integral_band", band) == pkg.OK
            nwork = L.mi_blur_integral_work_bytes(w, h, c, n, 1)
            assert nwork == R.work_bytes(img.shape, 2, band)
            S, Q = (torch_cuda.full((img.size,), -1, dtype=torch_cuda.int32, device="cuda") for _ in range(2))
            d_work = torch_cuda.full((nwork + 64,), 0x5A, dtype=torch_cuda.uint8, device="cuda")
            pkg.check(L.mi_blur_enqueue_integral(ptr, S.data_ptr(), Q.data_ptr(), w, h, c, n, d_work.data_ptr(), stream(torch_cuda)), "mi_blur_enqueue_integral")
            torch_cuda.cuda.synchronize()
            assert last(L) == R.INTEGRAL_TILED and bool((d_work[nwork:] == 0x5A).all())
            assert np.array_equal(S.cpu().numpy().view(np.uint32).reshape(img.shape), R.ref_integral(img)), band
            assert np.array_equal(Q.cpu().numpy().view(np.uint32).reshape(img.shape), R.ref_integral(img, True)), band
    finally:
        assert L.mi_blur_set_option(b"integral_band", B) == pkg.OK


# ---------------------------------------------------------------- the consumer
@pytest.mark.parametrize("w,h,channels", [(16, 4, (3,)), (48, 40, (1, 2, 3, 4)), (272, 260, (3,))])
def test_box_from_integral(pkg, L, torch_cuda, w, h, channels):
    """The three modes at every radius of the list; 16 x 4 is all border, 272 x 260 has an interior at r = 127."""
    rng = np.random.default_rng(300 + w)
    for c in channels:
        img = two_images(rng, h, w, c)
        assert R.box_takes_tiled(img.shape)
        d, ptr = upload(torch_cuda, img)
        _, _, _, tabs = device_tables(pkg, L, torch_cuda, ptr, img.shape)
        for rx, ry in RADII:
            for op in OPS:
                k = spec(pkg, op, rx, ry)
                want = R.ref_box(img, op, rx, ry, k.offset, k.invert)
                got = device_box(pkg, L, torch_cuda, ptr, tabs, img.shape, k)
                assert last(L) == R.BOX_TILED
                assert np.array_equal(got, want), (c, rx, ry, op)
                if (rx, ry) in ((1, 7), (127, 127)):
                    assert np.array_equal(cpu_box(pkg, L, img, k), want)


def test_box_other_launches_take_the_generic_kernel(pkg, L, torch_cuda):
    rng = np.random.default_rng(310)
    for h, w, c in ((9, 17, 1), (9, 17, 3), (6, 20, 3), (1, 1, 4), (40, 48, 3)):
        img = two_images(rng, h, w, c)
        d, ptr = upload(torch_cuda, img)
        _, _, _, tabs = device_tables(pkg, L, torch_cuda, ptr, img.shape)
        aligned = R.box_takes_tiled(img.shape)
        assert aligned == ((h, w, c) == (40, 48, 3))
        for rx, ry in ((1, 1), (2, 5), (127, 127)):
            for op in OPS:
                k = spec(pkg, op, rx, ry)
                want = R.ref_box(img, op, rx, ry, k.offset, k.invert)
                for off in ((0, 1, 7) if aligned else (0, 3)):
                    got = device_box(pkg, L, torch_cuda, ptr, tabs, img.shape, k, off)
                    assert last(L) == (R.BOX_TILED if aligned and off == 0 else R.BOX_GENERIC), (h, w, c, off)
                    assert np.array_equal(got, want), (h, w, c, rx, ry, op, off)
    # THRESHOLD reads the image: with the input 1 byte off the launch is generic too
    img = two_images(rng, 40, 48, 3)
    d, ptr = upload(torch_cuda, img, 1)
    _, _, _, tabs = device_tables(pkg, L, torch_cuda, ptr, img.shape)
    assert last(L) == R.INTEGRAL_GENERIC
    k = spec(pkg, R.THRESHOLD, 3, 3)
    assert np.array_equal(device_box(pkg, L, torch_cuda, ptr, tabs, img.shape, k), R.ref_box(img, R.THRESHOLD, 3, 3, k.offset, k.invert))
    assert last(L) == R.BOX_GENERIC
    assert np.array_equal(device_box(pkg, L, torch_cuda, ptr, tabs, img.shape, spec(pkg, R.MEAN, 3, 3)), R.ref_box(img, R.MEAN, 3, 3))
    assert last(L) == R.BOX_TILED                                                 # MEAN does not read it


def test_box_with_sixteen_bytes_per_thread(pkg, L, torch_cuda):
    """The A/B knob of the tiled consumer: threads that own 16 bytes give the same bytes."""
    rng = np.random.default_rng(311)
    img = two_images(rng, 60, 80, 3)
    d, ptr = upload(torch_cuda, img)
    _, _, _, tabs = device_tables(pkg, L, torch_cuda, ptr, img.shape)
    try:
        assert L.mi_blur_set_option(b"box_bytes", 16) == pkg.OK
        for op in OPS:
            for rx, ry in ((5, 3), (0, 0), (127, 127)):
                k = spec(pkg, op, rx, ry)
                assert np.array_equal(device_box(pkg, L, torch_cuda, ptr, tabs, img.shape, k), R.ref_box(img, op, rx, ry, k.offset, k.invert)), op
                assert last(L) == R.BOX_TILED
    finally:
        assert L.mi_blur_set_option(b"box_bytes", 4) == pkg.OK


def test_threshold_in_place(pkg, L, torch_cuda):
    rng = np.random.default_rng(312)
    for h, w, c, kernel in ((40, 48, 3, R.BOX_TILED), (9, 17, 3, R.BOX_GENERIC)):
        img = two_images(rng, h, w, c)
        d, ptr = upload(torch_cuda, img)
        _, _, _, tabs = device_tables(pkg, L, torch_cuda, ptr, img.shape)
        k = pkg.Box(R.THRESHOLD, 7, 2, 4, 0)
        device_box(pkg, L, torch_cuda, ptr, tabs, img.shape, k, in_place=True)
        assert last(L) == kernel
        o = d.cpu().numpy()
        assert np.array_equal(o[:img.size].reshape(img.shape), R.ref_box(img, R.THRESHOLD, 7, 2, 4, 0)) and not o[img.size:].any()


def test_fused_box_equals_the_two_calls(pkg, L, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(313)
    for h, w, c in ((70, 96, 3), (33, 21, 2), (2 * B + 1, 1040, 1)):
        img = two_images(rng, h, w, c)
        n = img.shape[0]
        d, ptr = upload(torch, img)
        _, _, _, tabs = device_tables(pkg, L, torch, ptr, img.shape)
        for op in OPS:
            k = spec(pkg, op, 9, 4)
            two = device_box(pkg, L, torch, ptr, tabs, img.shape, k)
            nwork = L.mi_blur_box_work_bytes(w, h, c, n, C.byref(k))
            table = (4 * img.size + 15) // 16 * 16
            tables = 2 if op == R.STDDEV else 1
            assert nwork == tables * table + R.work_bytes(img.shape, tables)
            d_work = torch.full((nwork + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            d_out = torch.full((img.size + 128,), 0x5A, dtype=torch.uint8, device="cuda")
            pkg.check(L.mi_blur_enqueue_box(ptr, d_out.data_ptr(), w, h, c, n, C.byref(k), d_work.data_ptr(), stream(torch)), "mi_blur_enqueue_box")
            torch.cuda.synchronize()
            o, wk = d_out.cpu().numpy(), d_work.cpu().numpy()
            assert (o[img.size:] == 0x5A).all() and (wk[nwork:] == 0x5A).all()
            assert np.array_equal(o[:img.size].reshape(img.shape), two) and np.array_equal(two, R.ref_box(img, op, 9, 4, k.offset, k.invert)), (h, w, c, op)
            assert np.array_equal(wk[:4 * img.size].view(np.uint32).reshape(img.shape), R.ref_integral(img))       # the work buffer starts with S
            if op == R.STDDEV:
                assert np.array_equal(wk[table:table + 4 * img.size].view(np.uint32).reshape(img.shape), R.ref_integral(img, True))
    # in place through the fused call
    img = two_images(rng, 40, 48, 3)
    d, ptr = upload(torch, img)
    k = pkg.Box(R.THRESHOLD, 5, 5, -6, 1)
    d_work = torch.empty((L.mi_blur_box_work_bytes(48, 40, 3, 2, C.byref(k)),), dtype=torch.uint8, device="cuda")
    pkg.check(L.mi_blur_enqueue_box(ptr, ptr, 48, 40, 3, 2, C.byref(k), d_work.data_ptr(), stream(torch)), "mi_blur_enqueue_box")
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy()[:img.size].reshape(img.shape), R.ref_box(img, R.THRESHOLD, 5, 5, -6, 1))


def test_numpy_functions_on_the_gpu(pkg, L, torch_cuda):
    rng = np.random.default_rng(314)
    stack = rng.integers(0, 256, size=(5, 90, 128, 3), dtype=np.uint8)
    odd = rng.integers(30, 200, size=(45, 71), dtype=np.uint8)
    odd4 = odd[None, :, :, None]
    assert np.array_equal(pkg.integral(stack, batch=2), R.ref_integral(stack)) and last(L) == R.INTEGRAL_TILED
    assert np.array_equal(pkg.integral(stack, square=True), R.ref_integral(stack, True)) and last(L) == R.INTEGRAL_TILED
    assert np.array_equal(pkg.integral(odd), R.ref_integral(odd4)[0, :, :, 0]) and last(L) == R.INTEGRAL_GENERIC
    assert pkg.rect_sum(pkg.integral(odd), 3, 4, 60, 40) == odd[4:41, 3:61].astype(np.int64).sum()
    assert np.array_equal(pkg.box_blur(stack, 31, batch=2), R.ref_box(stack, R.MEAN, 15, 15)) and last(L) == R.BOX_TILED
    assert np.array_equal(pkg.box_blur(stack, (255, 3)), R.ref_box(stack, R.MEAN, 127, 1))
    assert np.array_equal(pkg.local_stddev(stack, (7, 9)), R.ref_box(stack, R.STDDEV, 3, 4)) and last(L) == R.BOX_TILED
    assert np.array_equal(pkg.adaptive_threshold(stack, 201, 5), R.ref_box(stack, R.THRESHOLD, 100, 100, 5, 0)) and last(L) == R.BOX_TILED
    assert np.array_equal(pkg.adaptive_threshold(odd, 11, -3, True), R.ref_box(odd4, R.THRESHOLD, 5, 5, -3, 1)[0, :, :, 0]) and last(L) == R.BOX_GENERIC
    assert np.array_equal(pkg.local_stddev(odd, 5), R.ref_box(odd4, R.STDDEV, 2, 2)[0, :, :, 0])
    assert np.array_equal(pkg.box_blur(stack, 9), pkg.box_blur(stack, 9, device=pkg.DEVICE_CPU))
