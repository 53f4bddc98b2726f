"""The two-image arithmetic on the GPU (mi_blur_enqueue_arith, mi_blur_run_arith, arith() and its kin): exact bytes against
arith_ref.py and the CPU device, the definition over every operand pair and every LERP triple on the device, and which
kernel took each launch."""
import ctypes as C

import numpy as np
import pytest

import arith_ref as R
from arith_ref import FLAT, GENERIC, PLANE, PLANE_RUN, RUN
from resample_harness import last, torch_cuda  # noqa: F401
from table_harness import Guarded, stream, upload

pytestmark = pytest.mark.gpu

OPS = (R.LINEAR, R.ABSDIFF, R.MIN, R.MAX, R.MUL, R.LERP)
# units of a kernel per image: one; one below a workgroup's run, exactly a run, one above it; two runs plus one
UNITS = (1, RUN - 1, RUN, RUN + 1, 2 * RUN + 1)
UNIT_BLOCKS = (1, 1, 1, 2, 3)


def cpu_arith(pkg, L, k, a, b, m=None):
    out = np.empty_like(a)
    n, h, w, c = a.shape
    pkg.check(L.mi_blur_cpu_run_arith(a.ctypes.data, b.ctypes.data, None if m is None else m.ctypes.data, out.ctypes.data, w, h, c, n, C.byref(k), 4),
              "mi_blur_cpu_run_arith")
    return out


def gpu_arith(pkg, L, torch, k, a, b, m=None, off=(0, 0, 0, 0), alias=None):
    """mi_blur_enqueue_arith on a, b, m at off[0..2] bytes into their buffers.  The output lies off[3] bytes into a buffer
    of 0x5A with 128 bytes to spare, or is the buffer of a or b (alias = "a" | "b"); the spare bytes are checked."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    n, h, w, c = a.shape
    d_a, p_a = upload(torch, a, off[0])
    d_b, p_b = upload(torch, b, off[1])
    d_m, p_m = upload(torch, np.ascontiguousarray(m), off[2]) if m is not None else (None, None)
    if alias:
        d_out, p_out, o_off, fill = (d_a, p_a, off[0], 0) if alias == "a" else (d_b, p_b, off[1], 0)
    else:
        d_out = torch.full((a.size + 128,), 0x5A, dtype=torch.uint8, device="cuda")
        p_out, o_off, fill = d_out.data_ptr() + off[3], off[3], 0x5A
    pkg.check(L.mi_blur_enqueue_arith(p_a, p_b, p_m, p_out, w, h, c, n, C.byref(k), stream(torch)), "mi_blur_enqueue_arith")
    torch.cuda.synchronize()
    o = d_out.cpu().numpy()
    assert (o[:o_off] == fill).all() and (o[o_off + a.size:] == fill).all(), "wrote outside the output"
    return o[o_off:o_off + a.size].reshape(a.shape)


def check(pkg, L, torch, spec, a, b, m=None, kernel=None, want=None, **kw):
    """One launch against arith_ref and the CPU device; returns the struct."""
    k = R.struct_of(pkg, spec, b, m, a.shape)
    want = R.ref_arith(spec, a, b, m) if want is None else want
    got = gpu_arith(pkg, L, torch, k, a, b, m, **kw)
    if kernel:
        assert last(L) == kernel, (last(L), a.shape, spec)
    assert np.array_equal(got, want), (a.shape, spec, R.plane_flags(k, a.shape[3]), kw)
    assert np.array_equal(cpu_arith(pkg, L, k, a, b, m), want)
    return k


def all_pairs(c):
    """(1, 256, 256, c): a = the row, rotated by 85 per channel, so every channel sees every a; and the column as a plane."""
    row, col = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    a = np.stack([(row + 85 * ch) % 256 for ch in range(c)], axis=-1).astype(np.uint8)[None]
    return a, col.astype(np.uint8)[None, :, :, None]


def test_every_pair_on_the_flat_kernel(pkg, L, torch_cuda):
    a, b = all_pairs(1)
    rng = np.random.default_rng(150)
    m = rng.integers(0, 256, size=a.shape, dtype=np.uint8)
    specs = [row[1:] for row in R.PRESETS.values()] + [R.random_spec(rng, op) for op in OPS for _ in range(3)] + [R.lively_spec(rng, op) for op in OPS]
    for spec in specs:
        k = check(pkg, L, torch_cuda, spec, a, b, m if spec[0] == R.LERP else None, FLAT)
        assert R.takes_flat(a.shape, k) and R.blocks(a.shape, k) == 16


def test_every_pair_on_the_plane_kernel(pkg, L, torch_cuda):
    a, b = all_pairs(3)
    rng = np.random.default_rng(151)
    specs = [row[1:] for row in R.PRESETS.values() if row[1] != R.LERP] + [R.random_spec(rng, op) for op in OPS[:5] for _ in range(2)]
    for spec in specs:
        k = check(pkg, L, torch_cuda, spec, a, b, None, PLANE)
        assert R.takes_plane(a.shape, k) and R.blocks(a.shape, k) == 16


def test_lerp_every_triple_on_the_flat_kernel(pkg, L, torch_cuda):
    """All 2^24 (a, b, m) as one 4096 x 4096 x 1 launch."""
    idx = np.arange(1 << 24, dtype=np.int32).reshape(1, 4096, 4096, 1)
    a, b, m = ((idx >> s & 255).astype(np.uint8) for s in (16, 8, 0))
    t = a.astype(np.int32) * m + b.astype(np.int32) * (255 - m.astype(np.int32))
    want = ((2 * t + 255) // 510).astype(np.uint8)
    k = pkg.arith_preset("lerp")
    got = gpu_arith(pkg, L, torch_cuda, k, a, b, m)
    assert last(L) == FLAT and np.array_equal(got, want)
    assert np.array_equal(got[m == 255], a[m == 255]) and np.array_equal(got[m == 0], b[m == 0])


@pytest.mark.parametrize("c", [3, 4])
def test_lerp_every_pair_through_a_plane_mask(pkg, L, torch_cuda, c):
    a, m = all_pairs(c)
    for level in (0, 255, 100):
        b = np.empty_like(a)
        b[...] = (level + 37 * np.arange(c)) % 256
        check(pkg, L, torch_cuda, R.PRESETS["lerp"][1:], a, b, m, PLANE)
        check(pkg, L, torch_cuda, R.PRESETS["lerp"][1:], b, a, m, PLANE)


def flat_shapes():
    """(units per image, workgroups per image, (H, W, C)) with H * W * C = 16 * units, every C that divides that."""
    for units, nb in zip(UNITS, UNIT_BLOCKS):
        yield units, nb, (units, 16, 1)
        yield units, nb, (units, 8, 2)
        yield units, nb, (units, 4, 4)
        if units % 3 == 0:
            yield units, nb, (units // 3, 16, 3)


def test_flat_kernel_at_its_units(pkg, L, torch_cuda):
    rng = np.random.default_rng(152)
    for units, nb, (h, w, c) in flat_shapes():
        shape = (2, h, w, c)
        a = rng.integers(0, 256, size=shape, dtype=np.uint8)
        for op in OPS:
            spec = R.lively_spec(rng, op)
            b = R.operand(rng, shape, 0, 0)
            m = R.operand(rng, shape, 0, 0) if op == R.LERP else None
            k = check(pkg, L, torch_cuda, spec, a, b, m, FLAT)
            assert R.takes_flat(shape, k) and R.blocks(shape, k) == 2 * nb, (shape, units)


@pytest.mark.parametrize("c", [2, 3, 4])
def test_plane_kernel_at_its_units(pkg, L, torch_cuda, c):
    rng = np.random.default_rng(153 + c)
    for units, nb in zip((1, PLANE_RUN - 1, PLANE_RUN, PLANE_RUN + 1, 2 * PLANE_RUN + 1), UNIT_BLOCKS):
        shape = (2, units, 16, c)
        a = rng.integers(0, 256, size=shape, dtype=np.uint8)
        for op in OPS:
            for bp, mp in (((1, 0), (0, 1), (1, 1)) if op == R.LERP else ((1, 0),)):
                spec = R.lively_spec(rng, op)
                b = R.operand(rng, shape, bp, 0)
                m = R.operand(rng, shape, mp, 0) if op == R.LERP else None
                k = check(pkg, L, torch_cuda, spec, a, b, m, PLANE)
                assert R.takes_plane(shape, k) and R.blocks(shape, k) == 2 * nb, (shape, units)


def test_rows_that_are_not_whole_chunks(pkg, L, torch_cuda):
    """2 x 24 pixels: 24 c bytes a row, whole chunks only for c = 2 and 4; tiled all the same, the rule is flat."""
    rng = np.random.default_rng(157)
    for c in (1, 2, 3, 4):
        shape = (2, 2, 24, c)
        a = rng.integers(0, 256, size=shape, dtype=np.uint8)
        k = check(pkg, L, torch_cuda, R.PRESETS["absdiff"][1:], a, R.operand(rng, shape, 0, 0), None, FLAT)
        assert R.blocks(shape, k) == 2
        k = check(pkg, L, torch_cuda, R.PRESETS["lerp"][1:], a, R.operand(rng, shape, 0, 0), R.operand(rng, shape, 1, 0), PLANE if c > 1 else FLAT)
        assert R.blocks(shape, k) == 2


def own_ranges(rng, shape):
    """Images that each carry their own value range (16 values wide), so a swapped image shows."""
    n = shape[0]
    return (rng.integers(0, 16, size=shape) + 16 * np.arange(n).reshape(n, 1, 1, 1)).astype(np.uint8)


def test_batches_either_side_of_the_xcd_remap(pkg, L, torch_cuda):
    """Grids of 15 and of 18 workgroups: below 16 the blocks take the runs in order, from 16 on through the XCD remap."""
    rng = np.random.default_rng(158)
    for n in (5, 6):
        shape = (n, 3 * RUN, 16, 1)
        a, b = own_ranges(rng, shape), own_ranges(rng, shape)[::-1].copy()
        k = check(pkg, L, torch_cuda, R.PRESETS["sub"][1:], a, b, None, FLAT)
        assert R.blocks(shape, k) == 3 * n and (R.blocks(shape, k) >= 16) == (n == 6)
        shape = (n, 3 * PLANE_RUN, 16, 3)
        a, b, m = own_ranges(rng, shape), own_ranges(rng, shape)[::-1].copy(), own_ranges(rng, (n, 3 * PLANE_RUN, 16, 1))
        k = check(pkg, L, torch_cuda, R.PRESETS["lerp"][1:], a, b, m * 15, PLANE)
        assert R.blocks(shape, k) == 3 * n
        k = check(pkg, L, torch_cuda, R.PRESETS["add"][1:], a, m, None, PLANE)
        assert R.blocks(shape, k) == 3 * n


def test_shared_operands(pkg, L, torch_cuda):
    """n = 5: every image sees the same shared operand, whatever the other operand's form."""
    rng = np.random.default_rng(159)
    for shape in ((5, 40, 48, 3), (5, 40, 48, 1), (5, 7, 5, 3)):
        tiled = shape[1] * shape[2] % 16 == 0
        a = own_ranges(rng, shape)
        for op in (R.LINEAR, R.MUL):
            for bp in (0, 1):
                b = R.operand(rng, shape, bp, 1)
                k = check(pkg, L, torch_cuda, R.lively_spec(rng, op), a, b, None, GENERIC if not tiled else PLANE if bp and shape[3] > 1 else FLAT)
                assert k.b_shared == 1
        lerp = R.PRESETS["lerp"][1:]
        for (bp, bs), (mp, ms) in (((0, 1), (1, 0)), ((1, 0), (0, 1)), ((0, 1), (0, 1)), ((1, 1), (1, 1)), ((0, 0), (1, 1)), ((0, 1), (0, 0))):
            b, m = R.operand(rng, shape, bp, bs), R.operand(rng, shape, mp, ms)
            k = check(pkg, L, torch_cuda, lerp, a, b, m)
            assert (k.b_shared, k.m_shared) == (bs, ms)
            assert last(L) == ((PLANE if any(R.plane_flags(k, shape[3])) else FLAT) if tiled else GENERIC)
            # the same bytes with the shared operand repeated for every image
            full_b, full_m = np.broadcast_to(b, (5,) + b.shape[1:]).copy(), np.broadcast_to(m, (5,) + m.shape[1:]).copy()
            assert np.array_equal(R.ref_arith(lerp, a, b, m), R.ref_arith(lerp, a, full_b, full_m))


def test_other_launches_take_the_generic_kernel(pkg, L, torch_cuda):
    rng = np.random.default_rng(160)
    shape = (2, 33, 48, 3)
    a = rng.integers(0, 256, size=shape, dtype=np.uint8)
    add, lerp = R.PRESETS["add"][1:], R.PRESETS["lerp"][1:]
    b, m, pm = R.operand(rng, shape, 0, 0), R.operand(rng, shape, 0, 0), R.operand(rng, shape, 1, 0)
    check(pkg, L, torch_cuda, add, a, b, None, FLAT)
    check(pkg, L, torch_cuda, lerp, a, b, pm, PLANE)
    for delta in (1, 7, 3):
        for which in range(4):                                       # a, b, m, out in turn
            off = tuple(delta if i == which else 0 for i in range(4))
            k = check(pkg, L, torch_cuda, lerp, a, b, m, GENERIC, off=off)
            assert not R.takes_flat(shape, k, off)
            k = check(pkg, L, torch_cuda, lerp, a, b, pm, GENERIC, off=off)
            assert not R.takes_plane(shape, k, off)
            if which != 2:
                check(pkg, L, torch_cuda, add, a, b, None, GENERIC, off=off)
        check(pkg, L, torch_cuda, add, a, b, None, FLAT, off=(0, 0, delta, 0))          # no mask: its offset is nobody's
    # W * H * C no multiple of 16
    for c in (1, 2, 3, 4):
        odd = (2, 7, 5, c)
        x = rng.integers(0, 256, size=odd, dtype=np.uint8)
        for op in OPS:
            k = check(pkg, L, torch_cuda, R.lively_spec(rng, op), x, R.operand(rng, odd, 0, 0), R.operand(rng, odd, 0, 0) if op == R.LERP else None, GENERIC)
            assert not R.takes_flat(odd, k)
    # W * H no multiple of 16 with a plane operand while W * H * C is one: the flat kernel would read B wrongly
    for shape2 in ((2, 2, 4, 2), (2, 3, 4, 4), (3, 1, 8, 2)):
        x = rng.integers(0, 256, size=shape2, dtype=np.uint8)
        assert shape2[1] * shape2[2] * shape2[3] % 16 == 0 and shape2[1] * shape2[2] % 16 != 0
        k = check(pkg, L, torch_cuda, R.PRESETS["sub"][1:], x, R.operand(rng, shape2, 1, 0), None, GENERIC)
        assert not R.takes_plane(shape2, k) and not R.takes_flat(shape2, k)
        check(pkg, L, torch_cuda, lerp, x, R.operand(rng, shape2, 1, 1), R.operand(rng, shape2, 0, 0), GENERIC)
        check(pkg, L, torch_cuda, R.PRESETS["sub"][1:], x, R.operand(rng, shape2, 0, 0), None, FLAT)
    # one channel with the plane flags set: a full operand under another name
    grey = (3, 8, 10, 1)
    x, y, z = (rng.integers(0, 256, size=grey, dtype=np.uint8) for _ in range(3))
    for spec, mask in ((add, None), (lerp, z)):
        k = pkg.Arith(*spec, 1, 0, 1 if mask is not None else 0, 0)
        got = gpu_arith(pkg, L, torch_cuda, k, x, y, mask)
        assert last(L) == FLAT and R.takes_flat(grey, k) and np.array_equal(got, R.ref_arith(spec, x, y, mask))


def test_in_place(pkg, L, torch_cuda):
    rng = np.random.default_rng(161)
    lerp = R.PRESETS["lerp"][1:]
    for shape, kernel in (((3, 2 * RUN + 3, 16, 3), None), ((2, 7, 5, 3), GENERIC)):
        a, b = (rng.integers(0, 256, size=shape, dtype=np.uint8) for _ in range(2))
        m, pm = R.operand(rng, shape, 0, 0), R.operand(rng, shape, 1, 0)
        for alias in ("a", "b"):
            for op in (R.LINEAR, R.ABSDIFF, R.MUL):
                check(pkg, L, torch_cuda, R.lively_spec(rng, op), a, b, None, kernel or FLAT, alias=alias)
            check(pkg, L, torch_cuda, lerp, a, b, m, kernel or FLAT, alias=alias)
            check(pkg, L, torch_cuda, lerp, a, b, pm, kernel or PLANE, alias=alias)                  # B full, a plane mask
        check(pkg, L, torch_cuda, R.PRESETS["add"][1:], a, R.operand(rng, shape, 1, 0), None, kernel or PLANE, alias="a")
        check(pkg, L, torch_cuda, R.PRESETS["add"][1:], a, R.operand(rng, shape, 0, 1), None, kernel or FLAT, alias="a")
    # what the host tests refuse is refused here too, with a device present
    n, h, w, c = 2, 8, 8, 3
    d = torch_cuda.zeros(4 * n * h * w * c, dtype=torch_cuda.uint8, device="cuda")
    p, size = d.data_ptr(), n * h * w * c
    add, shared, plane, lp = pkg.arith_preset("add"), pkg.Arith(R.LINEAR, 1, 1, 0, 0, 0, 1), pkg.Arith(R.LINEAR, 1, 1, 0, 0, 1, 0), pkg.arith_preset("lerp")
    s = stream(torch_cuda)
    assert L.mi_blur_enqueue_arith(p + 16, p + 2 * size, None, p, w, h, c, n, C.byref(add), s) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_arith(p + 2 * size, p + size - 16, None, p, w, h, c, n, C.byref(add), s) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_arith(p + 2 * size, p, None, p, w, h, c, n, C.byref(shared), s) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_arith(p + 2 * size, p, None, p, w, h, c, n, C.byref(plane), s) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_arith(p + 2 * size, p + size, p, p, w, h, c, n, C.byref(lp), s) == pkg.ERR_INVALID
    torch_cuda.cuda.synchronize()
    assert not d.any().item()


def test_one_larger_image(pkg, L, torch_cuda):
    shape = (1, 1080, 1920, 3)
    a, b = np.empty(shape, np.uint8), np.empty(shape, np.uint8)
    L.mi_blur_fill_synthetic(a.ctypes.data, 1920, 1080, 3, 0, 1, 4)
    L.mi_blur_fill_synthetic(b.ctypes.data, 1920, 1080, 3, 1, 1, 4)
    m = np.random.default_rng(162).integers(0, 256, size=(1, 1080, 1920, 1), dtype=np.uint8)
    k = check(pkg, L, torch_cuda, R.PRESETS["absdiff"][1:], a, b, None, FLAT)
    assert R.blocks(shape, k) == -(-1080 * 1920 * 3 // 16 // RUN)
    k = check(pkg, L, torch_cuda, R.PRESETS["lerp"][1:], a, b, m, PLANE)
    assert R.blocks(shape, k) == -(-1080 * 1920 // 16 // PLANE_RUN)


def test_numpy_functions_on_the_gpu(pkg, L, torch_cuda):
    rng = np.random.default_rng(163)
    cpu = pkg.DEVICE_CPU
    a, b = (rng.integers(0, 256, size=(5, 36, 64, 3), dtype=np.uint8) for _ in range(2))
    mask = rng.integers(0, 256, size=(36, 64), dtype=np.uint8)
    k = pkg.Arith(R.LINEAR, 300, -200, 1000, 8)
    assert np.array_equal(pkg.arith(a, b, k, batch=2), pkg.arith(a, b, k, device=cpu)) and last(L) == FLAT
    assert np.array_equal(pkg.arith(a, b[0], k, batch=2), R.ref_arith(fields5(k), a, b[:1])) and last(L) == FLAT
    assert np.array_equal(pkg.arith(a, b[..., :1], k, batch=3), pkg.arith(a, b[..., :1], k, device=cpu)) and last(L) == PLANE
    got = pkg.blend(a, b, mask, batch=2)
    assert last(L) == PLANE and np.array_equal(got, pkg.blend(a, b, mask, device=cpu))
    assert np.array_equal(got, R.ref_arith(R.PRESETS["lerp"][1:], a, b, mask[None, :, :, None]))
    assert np.array_equal(pkg.blend(a, b, b), pkg.blend(a, b, b, device=cpu)) and last(L) == FLAT
    odd = rng.integers(0, 256, size=(45, 71), dtype=np.uint8)
    assert np.array_equal(pkg.absdiff(odd, odd[::-1].copy()), np.abs(odd.astype(int) - odd[::-1]).astype(np.uint8)) and last(L) == GENERIC
    assert np.array_equal(pkg.unsharp_mask(a, 1.5, 0.7, batch=2), pkg.unsharp_mask(a, 1.5, 0.7, device=cpu)) and last(L) == FLAT
    assert np.array_equal(pkg.unsharp_mask(odd, 1.0), pkg.unsharp_mask(odd, 1.0, device=cpu))
    assert np.array_equal(pkg.top_hat(a, 5), pkg.top_hat(a, 5, device=cpu))
    assert np.array_equal(pkg.difference_of_gaussians(a, 1.0, 2.0), pkg.difference_of_gaussians(a, 1.0, 2.0, device=cpu))


def fields5(k):
    return (k.op, k.wa, k.wb, k.bias, k.shift)
