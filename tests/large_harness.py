"""What tests/test_grid_caps_gpu.py, tests/test_large_shapes_newer_gpu.py and tests/test_large_refs_host.py share (not a test
module, and not a conftest): the shapes that lie past the grid caps of the generic kernels with the arithmetic that says
so, images whose first channel tells the images apart, the bands that hold a given byte, and one launch of the families
that filter_harness.py and resample_harness.py do not cover (arith, tables, integral, box from integral) with device
buffers inside guard patterns: 0x5A for bytes, 0xFFFFFFFF for words."""
import ctypes as C
import types

import numpy as np

import area_ref
import arith_ref
import box_ref
import color_ref
import hist_ref
import remap_ref
import resample_harness as rh
import resize_ref
import warp_perspective_ref as pr
import warp_ref as wr
from sep_down_ref import down_shape
from table_harness import stream, upload  # noqa: F401  (the tests take them as lh.stream, lh.upload)

BAND = 8                                        # rows of a compared band
ONES = 0xFFFFFFFF
GUARD_WORDS = 16                                # words in front of a table (64 bytes: the table stays 16-byte aligned) and behind it

# 3 x 2 796 711 = 8 390 133 bytes = 2 * (16384 * 256) + 1525: every thread of a capped byte-per-thread grid makes two trips
# and 1525 threads a third; 887 * 3 = 2661 is no multiple of 16 and 1051 * 887 is odd
BASE = (3, 1051, 887, 3)
DOWN_IN = (3, 2102, 1774, 3)                    # the inputs of the size-changing filters whose OUTPUT is BASE
RESIZE_IN = (3, 701, 591, 3)
AREA_IN = (3, 1400, 1183, 3)
GREY9 = (9, 1051, 887, 1)                       # 8 390 133 PIXELS: the colour transform has one thread per pixel
ROWS_SHAPE = (9, 29128, 5, 3)                   # 262 152 rows = 65536 * 4 + 8: two workgroups of 4 waves make a second trip
ROWS_REFUSED = (3, 87382, 5, 3)                 # 262 146 rows in 3 images: over the family's limit of 32768 rows an image
PARTS_SHAPE = (1, 1673, 1673, 3)                # 8 396 787 bytes in one image, 1673^2 odd


def own_ranges(rng, shape):
    """Random bytes; the first channel of image i lies in 16 i .. 16 i + 15, so output computed from a wrong image shows."""
    img = rng.integers(0, 256, size=shape, dtype=np.uint8)
    n = shape[0]
    assert n <= 16
    img[..., 0] = (img[..., 0] // 16 + 16 * np.arange(n).reshape(n, 1, 1)).astype(np.uint8)
    return img


def bands_of(shape, units, per_unit=None):
    """[(image, first row)] of bands of BAND rows of an (N, H, W, C) output: the first rows of image 0, and for every u of
    `units` the band around the row that holds the u-th unit of the launch (a unit is per_unit bytes: one byte, or the
    bytes of a pixel for a kernel with one thread per pixel)."""
    n, h, w, c = shape
    per_unit = per_unit or 1
    out = [(0, 0)]
    for u in units:
        img, rem = divmod(u * per_unit, h * w * c)
        assert img < n
        out.append((img, min(max(rem // (w * c) - BAND // 2, 0), h - BAND)))
    return out


def check_past_the_caps(cap, row_cap, hist_parts, part_bytes):
    """From the refs' eligibility rules and the caps given (the test files restate them from the source): the shapes above
    are past their caps, the trip boundaries of BASE fall inside images, and no fast path takes any of them."""
    n, h, w, c = BASE
    isz = h * w * c
    assert n * isz == 2 * cap + 1525 and GREY9[0] * GREY9[1] * GREY9[2] == n * isz
    assert isz < cap < 2 * isz - w * c                                        # byte `cap` lies inside image 1 ...
    assert 2 * isz < 2 * cap < 3 * isz and (2 * cap - 2 * isz) // (w * c) == h - 1   # ... and byte 2 cap in the last row of image 2
    assert (w * c) % 16 != 0 and (w * h) % 2 == 1                            # the rule of the same-size families: rows of whole chunks
    assert down_shape(DOWN_IN, 2, 2, 0, 0) == BASE
    assert not rh.SEP_DOWN.takes_tiled(DOWN_IN, (None, (2, 2, 0, 0)))
    for mode in (resize_ref.BILINEAR, resize_ref.NEAREST):
        assert not resize_ref.takes_tiled(RESIZE_IN, w, h, mode)
    for border in (wr.CLAMP, wr.CONSTANT):
        assert not wr.takes_tiled(BASE, wr.identity(), w, h, wr.BILINEAR, border)
        assert not pr.takes_tiled(BASE, pr.affine_h(wr.identity()), w, h, wr.BILINEAR, border)
    assert not remap_ref.takes_tiled(BASE, w, h)
    assert area_ref.valid(AREA_IN, w, h) and not area_ref.takes_tiled(AREA_IN, w, h)
    assert not color_ref.takes_tiled(GREY9) and not color_ref.takes_tiled(BASE)
    assert not hist_ref.takes_tiled(BASE)
    for b_plane, m_plane in ((0, 0), (1, 0), (0, 1)):
        k = types.SimpleNamespace(b_plane=b_plane, m_plane=m_plane)
        assert not arith_ref.takes_flat(BASE, k) and not arith_ref.takes_plane(BASE, k)
    assert not box_ref.box_takes_tiled(BASE) and not box_ref.integral_takes_tiled(BASE)
    assert w > 64                                                            # the generic integral's 64-pixel carry runs
    assert (h * w) % 16 != 0                                                 # the repack's 16-pixel kernel needs planes of whole groups
    rn, rh_, rw, rc = ROWS_SHAPE
    assert rn * rh_ == row_cap + 8 and rh_ <= area_ref.MAX_DIM and not box_ref.integral_takes_tiled(ROWS_SHAPE)
    assert (rn - 1) * rh_ < row_cap                                          # the trip boundary lies inside the last image
    assert ROWS_REFUSED[0] * ROWS_REFUSED[1] == row_cap + 2 and ROWS_REFUSED[1] > area_ref.MAX_DIM
    pn, ph, pw, pc = PARTS_SHAPE
    assert pn == 1 and ph * pw * pc == 8396787 > hist_parts * part_bytes and (ph * pw) % 2 == 1
    assert not hist_ref.takes_tiled(PARTS_SHAPE)


# ---------------------------------------------------------------- one launch
def guarded_bytes(torch, size, guard=64):
    """A device buffer of 0x5A with `guard` bytes either side of `size` bytes; (tensor, address of the data)."""
    d = torch.full((size + 2 * guard,), 0x5A, dtype=torch.uint8, device="cuda")
    assert d.data_ptr() % 16 == 0 and guard % 16 == 0
    return d, d.data_ptr() + guard


def guards_intact(d, size, guard=64):
    return bool((d[:guard] == 0x5A).all()) and bool((d[guard + size:] == 0x5A).all())


def gpu_arith(pkg, L, torch, k, a, b, m=None):
    """mi_blur_enqueue_arith on host operands, the output inside guard bytes; the output on the host."""
    n, h, w, c = a.shape
    (d_a, p_a), (d_b, p_b) = upload(torch, a), upload(torch, b)
    d_m, p_m = upload(torch, m) if m is not None else (None, None)
    d_out, p_out = guarded_bytes(torch, a.size)
    pkg.check(L.mi_blur_enqueue_arith(p_a, p_b, p_m, p_out, w, h, c, n, C.byref(k), stream(torch)), "mi_blur_enqueue_arith")
    torch.cuda.synchronize()
    assert guards_intact(d_out, a.size), "wrote outside the output"
    return d_out[64:64 + a.size].cpu().numpy().reshape(a.shape)


def cpu_arith(pkg, L, k, a, b, m, n_threads):
    out = np.empty_like(a)
    n, h, w, c = a.shape
    pkg.check(L.mi_blur_cpu_run_arith(a.ctypes.data, b.ctypes.data, None if m is None else m.ctypes.data, out.ctypes.data, w, h, c, n, C.byref(k), n_threads),
              "mi_blur_cpu_run_arith")
    return out


def gpu_tables(pkg, L, torch, img, tables):
    n, h, w, c = img.shape
    (d_in, p_in), (d_tab, p_tab) = upload(torch, img), upload(torch, np.ascontiguousarray(tables, dtype=np.uint8))
    d_out, p_out = guarded_bytes(torch, img.size)
    pkg.check(L.mi_blur_enqueue_tables(p_in, p_out, w, h, c, n, p_tab, stream(torch)), "mi_blur_enqueue_tables")
    torch.cuda.synchronize()
    assert guards_intact(d_out, img.size), "wrote outside the output"
    return d_out[64:64 + img.size].cpu().numpy().reshape(img.shape)


def device_tables(pkg, L, torch, ptr, shape, want_s=True, want_q=True):
    """mi_blur_enqueue_integral on the images at ptr: every table inside GUARD_WORDS words of 0xFFFFFFFF, the work buffer
    with 64 bytes of 0x5A behind it, all checked on the device.  [S, Q] as int32 device tensors of the table alone (None
    where not asked); they are views, so the buffers live as long as they do."""
    n, h, w, c = shape
    words = n * h * w * c
    bufs = [torch.full((words + 2 * GUARD_WORDS,), -1, dtype=torch.int32, device="cuda") if on else None for on in (want_s, want_q)]
    ptrs = [None if b is None else b.data_ptr() + 4 * GUARD_WORDS for b in bufs]
    both = int(want_s and want_q)
    nwork = L.mi_blur_integral_work_bytes(w, h, c, n, both)
    tiled = box_ref.integral_takes_tiled(shape, ptr % 16)
    assert nwork == box_ref.work_bytes(shape, 2 if both else 1)
    d_work = torch.full((nwork + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    assert all(p is None or p % 16 == 0 for p in ptrs) and d_work.data_ptr() % 16 == 0
    pkg.check(L.mi_blur_enqueue_integral(ptr, ptrs[0], ptrs[1], w, h, c, n, d_work.data_ptr(), stream(torch)), "mi_blur_enqueue_integral")
    torch.cuda.synchronize()
    assert rh.last(L) == (box_ref.INTEGRAL_TILED if tiled else box_ref.INTEGRAL_GENERIC)
    for b in bufs:
        if b is not None:
            assert bool((b[:GUARD_WORDS] == -1).all()) and bool((b[GUARD_WORDS + words:] == -1).all()), "wrote outside the table"
    assert bool((d_work[nwork:] == 0x5A).all()), "wrote outside the work buffer"
    del d_work
    return [None if b is None else b[GUARD_WORDS:GUARD_WORDS + words] for b in bufs]


def host_table(t, shape):
    return t.cpu().numpy().view(np.uint32).reshape(shape)


def device_box(pkg, L, torch, p_in, tabs, shape, k, offset_out=0):
    """mi_blur_enqueue_box_from_integral from the device tables `tabs` (S, Q): the output lies offset_out bytes behind the
    front guard of a buffer of 0x5A, and stays on the device: (N, H, W, C) uint8."""
    n, h, w, c = shape
    size = n * h * w * c
    d_out, p_out = guarded_bytes(torch, size + 16)
    pS, pQ = (None if t is None else t.data_ptr() for t in tabs)
    pkg.check(L.mi_blur_enqueue_box_from_integral(p_in if k.op == box_ref.THRESHOLD else None, pS, pQ if k.op == box_ref.STDDEV else None,
                                                  p_out + offset_out, w, h, c, n, C.byref(k), stream(torch)), "mi_blur_enqueue_box_from_integral")
    torch.cuda.synchronize()
    lo = 64 + offset_out
    assert bool((d_out[:lo] == 0x5A).all()) and bool((d_out[lo + size:] == 0x5A).all()), "wrote outside the output"
    return d_out[lo:lo + size].reshape(shape)


def box_spec(pkg, op, rx, ry):
    return pkg.Box(op, rx, ry, -3, rx & 1) if op == box_ref.THRESHOLD else pkg.Box(op, rx, ry, 0, 0)


def cpu_box(pkg, L, img, k, n_threads):
    out = np.empty_like(img)
    n, h, w, c = img.shape
    pkg.check(L.mi_blur_cpu_run_box(img.ctypes.data, out.ctypes.data, w, h, c, n, C.byref(k), n_threads), "mi_blur_cpu_run_box")
    return out
