"""CLAHE on the GPU (mi_blur_enqueue_clahe_tables, mi_blur_enqueue_clahe_apply, mi_blur_enqueue_clahe, clahe()): exact
tile histograms, tables and bytes against clahe_ref.py and the CPU device, and which kernel took each launch.  Outputs and
work buffers lie inside guard bytes of 0x5A, which are checked after every launch."""
import ctypes as C

import numpy as np
import pytest

from clahe_ref import (APPLY_GENERIC, APPLY_TILED, BINS, GENERIC_BLOCKS, LDS_TABLE_BYTES, TABLES_GENERIC, TABLES_TILED, apply_takes_tiled, ref_apply,
                       ref_clahe, ref_table, ref_tables, span_cols, split_work, tables_take_tiled, tile_box, work_words)
from resample_harness import last, torch_cuda  # noqa: F401
from table_harness import Guarded, stream, upload

pytestmark = pytest.mark.gpu

GUARD = 64
BYTE_CAP = 16384 * 256          # byte_grid(), csrc/kernel_common.h: workgroups x threads of blur_clahe_apply_generic_kernel
CPU_THREADS = 16


def gpu_tables(pkg, L, torch, img, tiles, clip_q8, mask=0, offset_in=0):
    """mi_blur_enqueue_clahe_tables: (hist, tables, the kernel's name); the work buffer ends in 64 bytes of 0x5A."""
    n, h, w, c = img.shape
    d_in, p_in = upload(torch, img, offset_in)
    words = work_words(n, tiles, c)
    d_work = Guarded(torch, 5 * words, "the work buffer", back=GUARD)
    k = pkg.Clahe(tiles[0], tiles[1], clip_q8, mask)
    pkg.check(L.mi_blur_enqueue_clahe_tables(p_in, w, h, c, n, C.byref(k), d_work.ptr, stream(torch)), "mi_blur_enqueue_clahe_tables")
    torch.cuda.synchronize()
    name = last(L)
    hist, tables = split_work(d_work.payload(), n, tiles, c)
    return hist, tables, name


def gpu_apply(pkg, L, torch, img, tiles, tables, offset_in=0, offset_out=0, offset_tab=0):
    """mi_blur_enqueue_clahe_apply: (output, the kernel's name); the output lies 64 + offset_out bytes into a buffer of 0x5A
    with as much behind it."""
    n, h, w, c = img.shape
    d_in, p_in = upload(torch, img, offset_in)
    d_tab, p_tab = upload(torch, np.ascontiguousarray(tables, dtype=np.uint8), offset_tab)
    d_out = Guarded(torch, img.size, "the output", front=GUARD + offset_out, back=GUARD + 16 - offset_out)
    k = pkg.Clahe(tiles[0], tiles[1], 0, 0)
    pkg.check(L.mi_blur_enqueue_clahe_apply(p_in, d_out.ptr, w, h, c, n, C.byref(k), p_tab, stream(torch)), "mi_blur_enqueue_clahe_apply")
    torch.cuda.synchronize()
    name = last(L)
    return d_out.payload().reshape(img.shape), name


def cpu_clahe(pkg, L, img, tiles, clip_q8, mask=0):
    n, h, w, c = img.shape
    k = pkg.Clahe(tiles[0], tiles[1], clip_q8, mask)
    out, wk = np.empty_like(img), np.empty(5 * work_words(n, tiles, c), np.uint8)
    pkg.check(L.mi_blur_cpu_run_clahe(img.ctypes.data, out.ctypes.data, w, h, c, n, C.byref(k), wk.ctypes.data, CPU_THREADS), "mi_blur_cpu_run_clahe")
    return (out,) + split_work(wk, n, tiles, c)


def perm_tables(rng, n, tiles, c):
    """A random permutation per image, tile and channel: a wrong tile, channel or weight shows."""
    return rng.permuted(np.tile(np.arange(BINS, dtype=np.uint8), (n, tiles[1], tiles[0], c, 1)), axis=-1)


def both_steps(pkg, L, torch, img, tiles, clip_q8, mask=0, tiled=True, **offsets):
    """Tables and apply on the GPU against the restatement and the CPU device; returns the GPU output."""
    want, want_hist, want_tables = ref_clahe(img, tiles, clip_q8, mask)
    cpu_out, cpu_hist, cpu_tables = cpu_clahe(pkg, L, img, tiles, clip_q8, mask)
    assert np.array_equal(cpu_hist, want_hist) and np.array_equal(cpu_tables, want_tables) and np.array_equal(cpu_out, want)
    off_in = offsets.get("offset_in", 0)
    hist, tables, name = gpu_tables(pkg, L, torch, img, tiles, clip_q8, mask, off_in)
    assert name == (TABLES_TILED if tiled and off_in % 16 == 0 else TABLES_GENERIC) and tables_take_tiled(img.shape, off_in) == (name == TABLES_TILED)
    assert np.array_equal(hist, want_hist), (img.shape, tiles, clip_q8)
    assert np.array_equal(tables, want_tables), (img.shape, tiles, clip_q8)
    got, name = gpu_apply(pkg, L, torch, img, tiles, tables, **offsets)
    assert apply_takes_tiled(img.shape, tiles, off_in, offsets.get("offset_out", 0)) == (name == APPLY_TILED)
    assert name == (APPLY_TILED if tiled and not any(o % 16 for o in offsets.values()) else APPLY_GENERIC)
    assert np.array_equal(got, want), (img.shape, tiles, clip_q8)
    return got


def images(rng, n, h, w, c):
    img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    img[0] = (60 + img[0] % 90).astype(np.uint8)                         # a low-contrast image: the clip bites
    return img


# (H, W, tiles, clips): one group; tile edges inside 16-byte chunks, so both neighbours mask the same chunk; one-pixel
# tiles; 9216 pixels in one tile: more than one sweep of a workgroup; whole groups per tile at three clips
SMALLEST = [(4, 16, (1, 1), (512,)), (9, 48, (3, 3), (512,)), (9, 48, (5, 2), (512,)), (16, 16, (16, 16), (512,)), (96, 96, (1, 1), (512,)),
            (40, 64, (8, 8), (0, 512, 65536))]


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_smallest_shapes_of_each_mechanism(pkg, L, torch_cuda, c):
    rng = np.random.default_rng(2450 + c)
    for h, w, tiles, clips in SMALLEST:
        img = images(rng, 2, h, w, c)
        for q in clips:
            both_steps(pkg, L, torch_cuda, img, tiles, q)
        both_steps(pkg, L, torch_cuda, img, tiles, 512, mask=1)
        tables = perm_tables(rng, 2, tiles, c)
        want = ref_apply(img, tables)
        for off in (0, 3):                                                # d_tables at any alignment
            got, name = gpu_apply(pkg, L, torch_cuda, img, tiles, tables, offset_tab=off)
            assert name == APPLY_TILED and np.array_equal(got, want), (h, w, tiles, off)


@pytest.mark.parametrize("c", [1, 3])
def test_flat_images_take_the_agree_paths(pkg, L, torch_cuda, c):
    """A constant image, and an image that is constant per tile (tiles of 32 x 16: whole groups, so whole waves agree)."""
    h, w, tiles = 64, 128, (4, 4)
    flat = np.full((2, h, w, c), 77, np.uint8)
    flat[1] = 200
    both_steps(pkg, L, torch_cuda, flat, tiles, 512)
    assert (both_steps(pkg, L, torch_cuda, flat, tiles, 0) == 255).all()   # without a clip c(v) = A at the only level present
    per_tile = np.empty((2, h, w, c), np.uint8)
    for j in range(4):
        for i in range(4):
            x0, x1, y0, y1 = tile_box(w, h, 4, 4, i, j)
            per_tile[:, y0:y1, x0:x1] = (16 * j + 3 * i + 40 * np.arange(2)[:, None, None, None] + np.arange(c)) % 256
    hist, tables, name = gpu_tables(pkg, L, torch_cuda, per_tile, tiles, 0)
    assert name == TABLES_TILED and (hist.max(axis=-1) == 32 * 16).all() and ((hist > 0).sum(axis=-1) == 1).all()
    both_steps(pkg, L, torch_cuda, per_tile, tiles, 0)
    half = np.array(per_tile)
    half[:, :, 1::2] = 9                                                  # every other pixel: no thread's 16 pixels agree
    both_steps(pkg, L, torch_cuda, half, tiles, 512)


def test_batches_either_side_of_the_xcd_remap(pkg, L, torch_cuda):
    """32 x 32 with tiles (3, 3): 9 table workgroups and 4 apply workgroups an image, so batches of 1, 2, 3 and 5 images
    launch 9 / 18 / 27 / 45 and 4 / 8 / 12 / 20: either side of 16 for both kernels.  Every image has its own range."""
    rng = np.random.default_rng(2460)
    for n in (1, 2, 3, 5):
        img = rng.integers(0, 256, size=(n, 32, 32, 3), dtype=np.uint8)
        img[..., 0] = (img[..., 0] // 8 + 32 * np.arange(n)[:, None, None]).astype(np.uint8)
        both_steps(pkg, L, torch_cuda, img, (3, 3), 512)
        tables = perm_tables(rng, n, (3, 3), 3)
        got, name = gpu_apply(pkg, L, torch_cuda, img, (3, 3), tables)
        assert name == APPLY_TILED and np.array_equal(got, ref_apply(img, tables)), n


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_other_launches_take_the_generic_kernels(pkg, L, torch_cuda, c):
    rng = np.random.default_rng(2470 + c)
    for h, w, tiles in ((9, 17, (3, 2)), (5, 7, (7, 5))):
        img = images(rng, 2, h, w, c)
        assert not tables_take_tiled(img.shape)
        both_steps(pkg, L, torch_cuda, img, tiles, 512, tiled=False)
        tables = perm_tables(rng, 2, tiles, c)
        got, name = gpu_apply(pkg, L, torch_cuda, img, tiles, tables, offset_tab=3)
        assert name == APPLY_GENERIC and np.array_equal(got, ref_apply(img, tables))
    img = images(rng, 2, 9, 48, c)
    tiled = both_steps(pkg, L, torch_cuda, img, (5, 2), 512)
    for off in (1, 7, 8):
        assert np.array_equal(both_steps(pkg, L, torch_cuda, img, (5, 2), 512, offset_in=off), tiled), off
    assert np.array_equal(both_steps(pkg, L, torch_cuda, img, (5, 2), 512, offset_out=8), tiled)


def test_the_lds_rule_of_the_tiled_apply(pkg, L, torch_cuda):
    """1024 x 2 x 4: the header's rule counts the tile columns a span of 256 pixels needs; the largest grid it admits runs
    on the tiled kernel and the next one on the generic kernel, with the same bytes as the restatement.  With 3 channels
    the finest grid still fits."""
    rng = np.random.default_rng(2480)
    h, w, c = 2, 1024, 4
    refused = min(tx for tx in range(1, 65) if not apply_takes_tiled((1, h, w, c), (tx, 1)))
    admitted = refused - 1
    assert span_cols(w, admitted) * 2 * c * BINS <= LDS_TABLE_BYTES < span_cols(w, refused) * 2 * c * BINS and 1 < refused <= 64
    assert apply_takes_tiled((1, h, w, 3), (64, 2)) and not apply_takes_tiled((1, h, w, c), (64, 2))
    for ch, tiles, tiled in ((c, (admitted, 2), True), (c, (refused, 2), False), (c, (64, 2), False), (3, (64, 2), True)):
        img = images(rng, 2, h, w, ch)
        tables = perm_tables(rng, 2, tiles, ch)
        got, name = gpu_apply(pkg, L, torch_cuda, img, tiles, tables)
        assert name == (APPLY_TILED if tiled else APPLY_GENERIC), (ch, tiles)
        assert np.array_equal(got, ref_apply(img, tables)), (ch, tiles)
        hist, tabs, name = gpu_tables(pkg, L, torch_cuda, img, tiles, 512)          # the tables kernel has no such rule
        want_hist, want_tabs = ref_tables(img, tiles, 512)
        assert name == TABLES_TILED and np.array_equal(hist, want_hist) and np.array_equal(tabs, want_tabs)


def test_generic_kernels_past_their_grid_caps(pkg, L, torch_cuda):
    """blur_clahe_tables_generic_kernel has at most GENERIC_BLOCKS workgroups: 5 images of 65 x 64 in 64 x 64 tiles are
    20480 jobs, so 4096 workgroups take a second tile.  blur_clahe_apply_generic_kernel runs under byte_grid(): one image
    of 2049 x 2049 is 4097 bytes past BYTE_CAP.  Whole outputs against the CPU device; the restatement on the tiles either
    side of the cap, and on the whole image for the apply."""
    rng = np.random.default_rng(2490)
    n, h, w, tiles = GENERIC_BLOCKS // 4096 + 1, 64, 65, (64, 64)
    jobs = n * tiles[0] * tiles[1]
    assert GENERIC_BLOCKS < jobs < 2 * GENERIC_BLOCKS and w % 16
    img = rng.integers(0, 256, size=(n, h, w, 1), dtype=np.uint8)
    hist, tables, name = gpu_tables(pkg, L, torch_cuda, img, tiles, 512)
    assert name == TABLES_GENERIC
    _, cpu_hist, cpu_tables = cpu_clahe(pkg, L, img, tiles, 512)
    assert np.array_equal(hist, cpu_hist) and np.array_equal(tables, cpu_tables)
    for job in (0, GENERIC_BLOCKS - 1, GENERIC_BLOCKS, GENERIC_BLOCKS + 1, jobs - 1):
        k, j, i = job // 4096, job % 4096 // 64, job % 64
        x0, x1, y0, y1 = tile_box(w, h, 64, 64, i, j)
        hh = np.bincount(img[k, y0:y1, x0:x1, 0].reshape(-1), minlength=BINS)
        assert np.array_equal(hist[k, j, i, 0], hh) and tables[k, j, i, 0].tolist() == ref_table(hh, (x1 - x0) * (y1 - y0), 512), job

    side = int(np.sqrt(BYTE_CAP)) + 1
    assert side * side > BYTE_CAP >= (side - 1) * (side - 1) and side % 16
    img = rng.integers(0, 256, size=(1, side, side, 1), dtype=np.uint8)
    cpu_out, _, cpu_tables = cpu_clahe(pkg, L, img, (8, 8), 512)
    got, name = gpu_apply(pkg, L, torch_cuda, img, (8, 8), cpu_tables)
    assert name == APPLY_GENERIC and np.array_equal(got, cpu_out) and np.array_equal(got, ref_apply(img, cpu_tables))


@pytest.mark.parametrize("c", [1, 3])
def test_end_to_end(pkg, L, torch_cuda, c):
    """mi_blur_enqueue_clahe = mi_blur_cpu_run_clahe = the restatement, work buffer and bytes, on the synthetic stream
    plus a low-contrast image; the images of a batch get different tables."""
    torch = torch_cuda
    n, h, w, tiles, q = 5, 240, 320, (8, 8), 512
    img = np.empty((n, h, w, c), np.uint8)
    L.mi_blur_fill_synthetic(img.ctypes.data, w, h, c, 0, 4, 4)
    img[4] = (90 + np.random.default_rng(2495).integers(0, 51, size=(h, w, c))).astype(np.uint8)
    words = work_words(n, tiles, c)
    k = pkg.Clahe(tiles[0], tiles[1], q, 0)
    assert L.mi_blur_clahe_work_bytes(w, h, c, n, C.byref(k)) == 5 * words
    want, want_hist, want_tables = ref_clahe(img, tiles, q)
    cpu_out, cpu_work = np.empty_like(img), np.empty(5 * words, np.uint8)
    pkg.check(L.mi_blur_cpu_run_clahe(img.ctypes.data, cpu_out.ctypes.data, w, h, c, n, C.byref(k), cpu_work.ctypes.data, CPU_THREADS), "mi_blur_cpu_run_clahe")
    d_in, p_in = upload(torch, img)
    d_out = torch.full((img.size + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    d_work = torch.full((5 * words + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    pkg.check(L.mi_blur_enqueue_clahe(p_in, d_out.data_ptr() + GUARD, w, h, c, n, C.byref(k), d_work.data_ptr(), stream(torch)), "mi_blur_enqueue_clahe")
    torch.cuda.synchronize()
    assert last(L) == APPLY_TILED
    o, wk = d_out.cpu().numpy(), d_work.cpu().numpy()
    assert (o[:GUARD] == 0x5A).all() and (o[GUARD + img.size:] == 0x5A).all() and (wk[5 * words:] == 0x5A).all()
    assert np.array_equal(wk[:5 * words], cpu_work)
    hist, tables = split_work(wk, n, tiles, c)
    assert np.array_equal(hist, want_hist) and np.array_equal(tables, want_tables)
    got = o[GUARD:GUARD + img.size].reshape(img.shape)
    assert np.array_equal(got, want) and np.array_equal(cpu_out, want)
    assert not np.array_equal(tables[3], tables[4]) and not np.array_equal(tables[0], tables[1])
    assert not np.array_equal(tables[0, 0, 0], tables[0, 3, 5])           # and the tiles of an image (of the stream: the noise of
    #                                                                       image 4 is clipped flat in every tile alike)
    for i in range(n):
        assert np.array_equal(got[i], ref_apply(img[i:i + 1], tables[i:i + 1])[0]), i


def test_numpy_functions_on_the_gpu(pkg, L, torch_cuda):
    rng = np.random.default_rng(2497)
    stack = images(rng, 5, 90, 128, 3)
    odd = rng.integers(30, 200, size=(45, 71), dtype=np.uint8)
    assert np.array_equal(pkg.clahe(stack, batch=2), ref_clahe(stack, (8, 8), 512)[0]) and last(L) == APPLY_TILED
    assert np.array_equal(pkg.clahe(odd, 3.0, (4, 3)), ref_clahe(odd[None, :, :, None], (4, 3), 768)[0][0, :, :, 0]) and last(L) == APPLY_GENERIC
    hist, tables = pkg.clahe_tables(stack, 2.0, (8, 8))
    want_hist, want_tables = ref_tables(stack, (8, 8), 512)
    assert np.array_equal(hist, want_hist) and np.array_equal(tables, want_tables)
    assert np.array_equal(pkg.clahe(stack, mode="luma"), pkg.clahe(stack, mode="luma", device=pkg.DEVICE_CPU))
