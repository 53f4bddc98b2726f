"""Erode / dilate / morphological gradient on a real MI355X (-m gpu): mi_blur_enqueue_morph / _band, a context given the
filter by mi_blur_ctx_set_morph, erode() / dilate() / morph_gradient() and the hosts' flags, byte for byte against a numpy
restatement of the definition in include/mi_blur.h and against the CPU device.

Inputs as in tests/test_morph_host.py: sparse impulses (more than 33 apart, one channel each, on the image's edges and on
both sides of every tile seam of blur_morph_tiled_kernel and of the slots a wave stages), ramps, checkerboards and
low-amplitude noise at every radius; random bytes at the small radii only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

pytestmark = pytest.mark.gpu

ERODE, DILATE, GRADIENT = 0, 1, 2
OPS = (ERODE, DILATE, GRADIENT)
TILED, GENERIC = "blur_morph_tiled_kernel", "blur_morph_generic_kernel"
TILE_ROWS, TILE_CHUNKS = 32, 32                                   # blur_morph_tiled_kernel's tile: output rows x 16-byte chunk columns


def _finish(lo, hi, op):
    return lo if op == ERODE else hi if op == DILATE else (hi.astype(np.int16) - lo.astype(np.int16)).astype(np.uint8)


def ref_morph_2d(img, op, rx, ry):
    """The definition: img (N, H, W, C) uint8, edge padding by (ry, rx), min / max over every full 2-D window."""
    p = np.pad(img, ((0, 0), (ry, ry), (rx, rx), (0, 0)), mode="edge")
    win = sliding_window_view(p, (2 * ry + 1, 2 * rx + 1), axis=(1, 2))
    return _finish(win.min(axis=(-2, -1)), win.max(axis=(-2, -1)), op)


def ref_lo_hi(img, rx, ry):
    """The separable restatement (1-D windows along x, then along y), tied to the 2-D one by the first test."""
    p = np.pad(img, ((0, 0), (0, 0), (rx, rx), (0, 0)), mode="edge")
    wx = sliding_window_view(p, 2 * rx + 1, axis=2)
    lo, hi = wx.min(axis=-1), wx.max(axis=-1)
    lo = sliding_window_view(np.pad(lo, ((0, 0), (ry, ry), (0, 0), (0, 0)), mode="edge"), 2 * ry + 1, axis=1).min(axis=-1)
    hi = sliding_window_view(np.pad(hi, ((0, 0), (ry, ry), (0, 0), (0, 0)), mode="edge"), 2 * ry + 1, axis=1).max(axis=-1)
    return lo, hi


def ref_morph(img, op, rx, ry):
    return _finish(*ref_lo_hi(img, rx, ry), op)


def impulse_batch(h, w, c, candidates):
    """Images of 128 with single pixels of 0 / 255 (alternating) in one channel each at the candidate (y, x) positions;
    positions closer than 34 in both axes go to different images, so every image's impulses are more than 33 apart."""
    images = []
    for k, (y, x) in enumerate(dict.fromkeys((min(max(y, 0), h - 1), min(max(x, 0), w - 1)) for y, x in candidates)):
        for img, taken in images:
            if all(max(abs(y - yy), abs(x - xx)) > 33 for yy, xx in taken):
                break
        else:
            img, taken = np.full((h, w, c), 128, np.uint8), []
            images.append((img, taken))
        img[y, x, k % c] = 0 if k % 2 else 255
        taken.append((y, x))
    return np.stack([img for img, _ in images])


def seam_impulses(h, w, c, rx, ry):
    """Impulses on the image's edges, on both sides of every seam between tiles (rows and chunk columns) and in the first and
    last 16-byte chunk of the 64-slot groups one wave stages (slot = staged row * staged chunk columns + chunk)."""
    cpr = w * c // 16
    nstrips = -(-cpr // TILE_CHUNKS) if cpr else 1
    ncols = -(-cpr // nstrips) if cpr else 1
    hc = max(1, -(-rx * c // 16))
    rows = sorted({0, h - 1, h // 2} | {y for s in range(TILE_ROWS, h, TILE_ROWS) for y in (s - 1, s)})
    cols = sorted({0, w - 1, w // 2} | {x for s in range(ncols, cpr, ncols) for x in ((s * 16 - 1) // c, -(-s * 16 // c))})
    cand = [(y, x) for y in rows for x in cols]
    ncw = min(ncols, cpr) + 2 * hc
    for s in (63, 64, 127, 128, 64 * ((TILE_ROWS + 2 * ry) * ncw // 64) - 1, 64 * ((TILE_ROWS + 2 * ry) * ncw // 64)):
        row, cc = divmod(s, ncw)
        for b in (0, 15):
            cand.append((row - ry, ((cc - hc) * 16 + b) // c))   # first tile: staged row 0 is image row -ry (clamped away)
    return impulse_batch(h, w, c, cand)


def structured(rng, n, h, w, c):
    yy, xx = np.mgrid[0:h, 0:w]
    return [np.broadcast_to(((xx * 7 + yy * 3) % 256).astype(np.uint8)[None, :, :, None], (n, h, w, c)).copy(),
            np.broadcast_to((((xx + yy) % 2) * 255).astype(np.uint8)[None, :, :, None], (n, h, w, c)).copy(),
            rng.integers(100, 141, size=(n, h, w, c), dtype=np.uint8)]


def mixed(rng, n, h, w, c):
    """One batch with everything in it: low-amplitude noise, a ramp, a checkerboard, sparse salt and pepper on top."""
    yy, xx = np.mgrid[0:h, 0:w]
    img = rng.integers(100, 141, size=(n, h, w, c), dtype=np.uint8)
    img[0] = ((xx * 7 + yy * 3) % 256).astype(np.uint8)[:, :, None]
    if n > 1:
        img[1, : h // 2] = (((xx + yy) % 2) * 255).astype(np.uint8)[: h // 2, :, None]
    sp = rng.random((n, h, w, c)) < 0.002
    img[sp] = rng.choice(np.array([0, 255], np.uint8), int(sp.sum()))
    return img


@pytest.fixture(scope="module")
def torch_cuda(L):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert L.mi_blur_device_count() >= 1, "libmi_blur.so sees no HIP device"
    torch.cuda.set_device(0)
    return torch


def gpu_morph(pkg, L, torch, host, op, rx, ry, offset_in=0, offset_out=0, y0=None, y1=None):
    """host: N x H x W x C -> mi_blur_enqueue_morph (or _band for one image with y0/y1), guard bytes around the output."""
    n, h, w, c = host.shape
    y0 = 0 if y0 is None else y0
    y1 = h if y1 is None else y1
    size_out = n * (y1 - y0) * w * c
    d_in = torch.zeros(host.size + 64, dtype=torch.uint8, device="cuda")
    d_in[offset_in:offset_in + host.size] = torch.from_numpy(np.ascontiguousarray(host).reshape(-1)).cuda()
    d_out = torch.full((size_out + 128,), 0x5A, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if y0 == 0 and y1 == h:
        rc = L.mi_blur_enqueue_morph(d_in.data_ptr() + offset_in, d_out.data_ptr() + offset_out, w, h, c, op, rx, ry, n, s)
    else:
        assert n == 1
        rc = L.mi_blur_enqueue_morph_band(d_in.data_ptr() + offset_in, d_out.data_ptr() + offset_out, w, h, c, op, rx, ry, y0, y1, s)
    pkg.check(rc, "mi_blur_enqueue_morph")
    torch.cuda.synchronize()
    o = d_out.cpu().numpy()
    assert (o[:offset_out] == 0x5A).all() and (o[offset_out + size_out:] == 0x5A).all(), "wrote outside the output"
    return o[offset_out:offset_out + size_out].reshape(n, y1 - y0, w, c)


def test_separable_restatement_is_the_2d_definition():
    rng = np.random.default_rng(0)
    for (n, h, w, c) in ((2, 9, 13, 3), (1, 40, 37, 1)):
        for img in [impulse_batch(h, w, c, [(0, 0), (h - 1, w - 1), (h // 2, w // 3)])] + structured(rng, n, h, w, c):
            for rx in (0, 1, 2, 5, 16):
                for ry in (0, 1, 2, 5, 16):
                    for op in OPS:
                        assert np.array_equal(ref_morph(img, op, rx, ry), ref_morph_2d(img, op, rx, ry)), ((n, h, w, c), op, rx, ry)


# rows of whole 16-byte chunks with 1-4 channels (the tiled kernel at every radius) and everything else
ALIGNED = [(2, 64, 80, 3), (1, 40, 64, 4), (3, 33, 16, 1), (1, 100, 1024, 1), (1, 37, 2000, 4), (2, 70, 96, 2),
           (1, 1, 16, 1), (1, 2, 48, 1), (1, 300, 512, 3), (1, 5, 32, 2)]
RAGGED = [(1, 17, 33, 3), (2, 30, 250, 3), (1, 9, 5, 1), (1, 31, 29, 2), (1, 50, 7, 5), (1, 24, 64, 5), (1, 1, 1, 3),
          (1, 12, 16, 6), (1, 10, 20, 7), (1, 14, 18, 8)]
PAIRS = [(0, 0), (1, 1), (2, 2), (3, 0), (0, 3), (4, 5), (7, 8), (9, 3), (5, 12), (16, 15), (13, 16), (16, 16)]


def test_enqueue_morph_matches_numpy(pkg, L, torch_cuda):
    rng = np.random.default_rng(2024)
    for shapes, kern in ((ALIGNED, TILED), (RAGGED, GENERIC)):
        for (n, h, w, c) in shapes:
            imgs = [seam_impulses(h, w, c, 16, 16), mixed(rng, n, h, w, c)]
            rnd = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
            for rx, ry in PAIRS:
                for k, img in enumerate(imgs + ([rnd] if max(rx, ry) <= 2 else [])):
                    lo, hi = ref_lo_hi(img, rx, ry)
                    for op in OPS:
                        got = gpu_morph(pkg, L, torch_cuda, img, op, rx, ry)
                        assert L.mi_blur_last_kernel().decode() == kern, ((n, h, w, c), op, rx, ry)
                        assert np.array_equal(got, _finish(lo, hi, op)), ((n, h, w, c), op, rx, ry, k)


def test_every_radius_on_impulses(pkg, L, torch_cuda):
    """rx and ry each through 0..16 (the other at a fixed value): exact rectangles around impulses at seams and edges."""
    rng = np.random.default_rng(7)
    for (h, w, c) in ((70, 688, 3), (66, 1040, 1), (40, 272, 4), (35, 528, 2)):
        noise = rng.integers(100, 141, size=(1, h, w, c), dtype=np.uint8)
        for r in range(17):
            for rx, ry in ((r, 2), (3, r), (r, r)):
                img = np.concatenate([seam_impulses(h, w, c, rx, ry), noise])
                lo, hi = ref_lo_hi(img, rx, ry)
                for op in OPS:
                    got = gpu_morph(pkg, L, torch_cuda, img, op, rx, ry)
                    assert L.mi_blur_last_kernel().decode() == TILED
                    assert np.array_equal(got, _finish(lo, hi, op)), ((h, w, c), op, rx, ry)


def test_tile_edges(pkg, L, torch_cuda):
    """Heights and widths around the tile's row and chunk-column counts (one less, equal, one more, two tiles plus one),
    at radii on both sides of every power of two up to 16."""
    rng = np.random.default_rng(8)
    radii = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16)
    for c in (1, 3):
        for k, h in enumerate((TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, 2 * TILE_ROWS + 1)):
            for j, chunks in enumerate((TILE_CHUNKS - 1, TILE_CHUNKS, TILE_CHUNKS + 1, 2 * TILE_CHUNKS + 1)):
                cpr = chunks * c                                 # rows of whole chunks whatever the channel count
                w = cpr * 16 // c
                img = np.concatenate([seam_impulses(h, w, c, 16, 16), mixed(rng, 1, h, w, c)])
                for i, r in enumerate(radii):
                    rx, ry = (r, radii[(i + 3) % len(radii)]) if (k + j) % 2 else (r, r)
                    op = OPS[(i + k + j) % 3]
                    got = gpu_morph(pkg, L, torch_cuda, img, op, rx, ry)
                    assert L.mi_blur_last_kernel().decode() == TILED
                    assert np.array_equal(got, ref_morph(img, op, rx, ry)), ((h, w, c), op, rx, ry)


def test_enqueue_morph_unaligned_pointers(pkg, L, torch_cuda):
    rng = np.random.default_rng(5)
    img = mixed(rng, 2, 40, 64, 3)
    for op, rx, ry in ((ERODE, 1, 1), (DILATE, 6, 2), (GRADIENT, 16, 9)):
        want = ref_morph(img, op, rx, ry)
        assert np.array_equal(gpu_morph(pkg, L, torch_cuda, img, op, rx, ry), want)
        assert L.mi_blur_last_kernel().decode() == TILED
        for oi, oo in ((1, 0), (0, 7), (3, 5)):
            assert np.array_equal(gpu_morph(pkg, L, torch_cuda, img, op, rx, ry, oi, oo), want), (op, oi, oo)
            assert L.mi_blur_last_kernel().decode() == GENERIC


def test_bands_inside_the_image(pkg, L, torch_cuda):
    rng = np.random.default_rng(12)
    for (h, w, c) in ((64, 80, 3), (37, 17, 3), (90, 64, 4), (40, 48, 1)):
        img = mixed(rng, 1, h, w, c)
        for op, rx, ry in ((ERODE, 1, 1), (DILATE, 2, 4), (GRADIENT, 7, 2), (ERODE, 3, 16), (DILATE, 16, 0)):
            whole = ref_morph(img, op, rx, ry)
            for y0, y1 in ((ry, h - ry), (0, h // 2), (h // 3, h), (5, 6)):
                if y0 >= y1:
                    continue
                got = gpu_morph(pkg, L, torch_cuda, img, op, rx, ry, y0=y0, y1=y1)
                assert np.array_equal(got, whole[:, y0:y1]), (h, w, c, op, rx, ry, y0, y1)
            for split in (max(ry, 1), h // 2, h - max(ry, 1)):     # a band split with halo ry, joined, is the whole image
                top_rows = min(h, split + ry)
                top = gpu_morph(pkg, L, torch_cuda, np.ascontiguousarray(img[:, :top_rows]), op, rx, ry, y0=0, y1=split)
                b0 = max(split - ry, 0)
                bot = gpu_morph(pkg, L, torch_cuda, np.ascontiguousarray(img[:, b0:]), op, rx, ry, y0=split - b0, y1=h - b0)
                assert np.array_equal(np.concatenate([top, bot], axis=1), whole), (h, w, c, op, rx, ry, split)


def test_enqueue_morph_refusals(pkg, L, torch_cuda):
    d = torch_cuda.zeros(4096, dtype=torch_cuda.uint8, device="cuda")
    p, q = d.data_ptr(), d.data_ptr() + 2048
    for op in (-1, 3):
        assert L.mi_blur_enqueue_morph(p, q, 16, 8, 3, op, 1, 1, 1, None) == pkg.ERR_INVALID
    for rx, ry in ((-1, 0), (0, -1), (17, 0), (0, 17)):
        assert L.mi_blur_enqueue_morph(p, q, 16, 8, 3, ERODE, rx, ry, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph(p, p, 16, 8, 3, ERODE, 1, 1, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph(None, q, 16, 8, 3, ERODE, 1, 1, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph(p, q, 0, 8, 3, ERODE, 1, 1, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph(p, q, 16, 8, 3, ERODE, 1, 1, -1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph_band(p, q, 16, 8, 3, DILATE, 1, 1, 6, 2, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph_band(p, q, 16, 8, 3, DILATE, 1, 1, 0, 9, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_morph(p, q, 16, 8, 3, GRADIENT, 16, 16, 0, None) == pkg.OK


def test_batch_over_2gib(pkg, L, torch_cuda):
    """A batch of more than 2^31 bytes: 64-bit image offsets, the last image checked."""
    torch = torch_cuda
    rng = np.random.default_rng(8)
    img = mixed(rng, 1, 1024, 1024, 3)
    n = 720                                                   # 2.26 GB in, as much out
    d_in = torch.from_numpy(img[0]).cuda().unsqueeze(0).repeat(n, 1, 1, 1)
    d_in[n - 1, 100:200, 300:400] = 255                       # the last image differs from the others
    last = d_in[n - 1].cpu().numpy()[None]
    d_out = torch.zeros_like(d_in)
    for op, rx, ry in ((ERODE, 2, 2), (GRADIENT, 9, 5)):
        pkg.check(L.mi_blur_enqueue_morph(d_in.data_ptr(), d_out.data_ptr(), 1024, 1024, 3, op, rx, ry, n, None))
        torch.cuda.synchronize()
        assert L.mi_blur_last_kernel().decode() == TILED
        want0 = torch.from_numpy(ref_morph(img, op, rx, ry)[0]).cuda()
        for i in (0, n // 2, n - 2):
            assert bool((d_out[i] == want0).all()), (op, i)
        assert np.array_equal(d_out[n - 1].cpu().numpy(), ref_morph(last, op, rx, ry)[0]), op
    del d_in, d_out
    torch.cuda.empty_cache()


def test_gpu_and_cpu_agree_on_the_synthetic_stream(pkg, L, torch_cuda):
    n, h, w, c = 1000, 256, 256, 3
    host = np.empty((n, h, w, c), np.uint8)
    L.mi_blur_fill_synthetic(host.ctypes.data, w, h, c, 0, n, 8)
    for op in OPS:
        for r in (1, 4, 16):
            want = np.empty_like(host)
            pkg.check(L.mi_blur_cpu_run_morph(host.ctypes.data, want.ctypes.data, w, h, c, op, r, r, n, 16))
            got = gpu_morph(pkg, L, torch_cuda, host, op, r, r)
            assert np.array_equal(got, want), (op, r)


def test_context_with_a_morph(pkg, L, torch_cuda):
    """Every submit form of a GPU context takes the filter: pageable, pinned (one launch: not the batch server), strided
    bands, one band, planar."""
    rng = np.random.default_rng(21)
    n, h, w, c = 6, 240, 320, 3                                # 1.38 MB of output per submit: the server size class
    img = mixed(rng, n, h, w, c)
    isz = img[0].size
    for op, rx, ry in ((ERODE, 1, 1), (DILATE, 4, 2), (GRADIENT, 16, 16)):
        want = ref_morph(img, op, rx, ry)
        with pkg.Context(0, w, h, c, 1, max_batch=n, n_slots=3) as ctx:
            ctx.set_morph(op, rx, ry)
            out = np.zeros_like(img)
            ctx.submit(img.ctypes.data, out.ctypes.data, n)
            ctx.sync()
            assert np.array_equal(out, want)
            assert L.mi_blur_last_kernel().decode() == TILED
            pin_in, pin_out = L.mi_blur_host_alloc(img.size), L.mi_blur_host_alloc(img.size)
            try:
                a = np.ctypeslib.as_array((C.c_uint8 * img.size).from_address(pin_in)).reshape(img.shape)
                b = np.ctypeslib.as_array((C.c_uint8 * img.size).from_address(pin_out)).reshape(img.shape)
                a[:] = img
                z0 = L.mi_blur_zero_copy_launches(ctx.h)
                for _ in range(2):
                    b[:] = 0
                    ctx.submit(pin_in, pin_out, n)
                    ctx.sync()
                    assert np.array_equal(b, want)
                assert L.mi_blur_zero_copy_launches(ctx.h) == z0 + 2
                assert L.mi_blur_last_kernel().decode() == TILED
            finally:
                L.mi_blur_host_free(pin_in)
                L.mi_blur_host_free(pin_out)
            bo = np.zeros_like(img)
            pitch = w * c
            ctx.submit_bands(img.ctypes.data + (60 - ry) * pitch, bo.ctypes.data + 60 * pitch, n, isz, 120 + 2 * ry, ry, ry)
            ctx.sync()
            assert np.array_equal(bo[:, 60:180], want[:, 60:180]) and not bo[:, :60].any() and not bo[:, 180:].any()
            so = np.zeros((100, w, c), np.uint8)
            ctx.submit_band(img[1].ctypes.data + (50 - ry) * pitch, so.ctypes.data, 100 + 2 * ry, ry, ry)
            ctx.sync()
            assert np.array_equal(so, want[1, 50:150])
            planar = np.ascontiguousarray(img.transpose(0, 3, 1, 2))
            po = np.zeros_like(img)
            ctx.submit_planar(planar.ctypes.data, po.ctypes.data, n)
            ctx.sync()
            assert np.array_equal(po, want)
            assert L.mi_blur_ctx_set_morph(ctx.h, op, rx, ry) == pkg.ERR_STATE
            ctx.resident_alloc(2)
            assert L.mi_blur_resident_run(ctx.h, 2, 1, 0) == pkg.ERR_UNSUPPORTED
            assert L.mi_blur_resident_run_fused(ctx.h, 2, 1, 0) == pkg.ERR_UNSUPPORTED


def test_morphology_functions_python(pkg, torch_cuda):
    rng = np.random.default_rng(30)
    imgs = mixed(rng, 4, 90, 128, 3)
    for fn, op in ((pkg.erode, ERODE), (pkg.dilate, DILATE), (pkg.morph_gradient, GRADIENT)):
        for k in (1, 3, 7, 17, 33):
            assert np.array_equal(fn(imgs, k), ref_morph(imgs, op, k // 2, k // 2)), (op, k)
        assert np.array_equal(fn(imgs, (9, 3), batch=3), ref_morph(imgs, op, 4, 1)), op
        g = imgs[0, :, :, 0]
        assert np.array_equal(fn(g, (5, 21)), ref_morph(g[None, :, :, None], op, 2, 10)[0, :, :, 0])


def write_ppm(path, img):
    h, w, _ = img.shape
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(img.tobytes())


def read_ppm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"P6"
        w, h = map(int, f.readline().split())
        assert f.readline().strip() == b"255"
        return np.frombuffer(f.read(), np.uint8).reshape(h, w, 3)


def test_hosts_morph_on_the_gpu(pkg, torch_cuda, tmp_path):
    pkg.build_native()
    het, spl = os.path.join(pkg.APPS, "heterogeneous_blur"), os.path.join(pkg.APPS, "split_image_blur")
    rng = np.random.default_rng(40)
    img = mixed(rng, 1, 240, 320, 3)[0]
    write_ppm(tmp_path / "in.ppm", img)
    for flag, k, op, name in (("--erode", 5, ERODE, "erode"), ("--dilate", 7, DILATE, "dilate"),
                              ("--morph-gradient", 33, GRADIENT, "morphological gradient")):
        want = ref_morph(img[None], op, k // 2, k // 2)[0]
        for mode in ("gpu", "both"):
            out = f"{mode}{k}.ppm"
            r = subprocess.run([het, mode, "0.7", "35", "--image", "in.ppm", "--images", "100", flag, str(k), "--save", out],
                               cwd=tmp_path, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout + r.stderr
            assert f"Blur kernel: {k}x{k} {name}\n" in r.stdout
            assert np.array_equal(read_ppm(tmp_path / out), want), (mode, flag)
    r = subprocess.run([spl, "0.6", "16", "--image", "in.ppm", "--images", "48", "--dilate", "7", "--save", "s.ppm"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Halo size: 3 row(s)" in r.stdout and "Blur kernel: 7x7 dilate\n" in r.stdout
    assert np.array_equal(read_ppm(tmp_path / "s.ppm"), ref_morph(img[None], DILATE, 3, 3)[0])
