"""Signed 2-D convolution on a real MI355X (-m gpu): mi_blur_enqueue_conv / _band, a context given the filter by
mi_blur_ctx_set_conv, filter2d() / sobel() / ... and the hosts' --conv, byte for byte against the numpy restatement of the
definition in include/mi_blur.h (conv_ref.py) and against the CPU device.  0x5A guard bytes surround every output."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conv_ref as cr
from conv_ref import ref_conv

pytestmark = pytest.mark.gpu

TILED, GENERIC = "blur_conv_tiled_kernel", "blur_conv_generic_kernel"
TILE_ROWS, TILE_CHUNKS = 32, 32                                   # blur_conv_tiled_kernel's tile: output rows x 16-byte chunk columns
# every rx (the column classes are 0-1, 2, 3, 4-5, 6-7) with a spread of ry
PAIRS = [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (7, 7), (0, 3), (1, 7), (2, 0), (3, 5), (4, 1), (5, 2), (6, 4), (7, 6)]
SOBEL_X = [[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]]
SOBEL = dict(K=SOBEL_X, mode="mag", K2=np.array(SOBEL_X).T.tolist())
SHARPEN = dict(K=[[0, -1, 0], [-1, 5, -1], [0, -1, 0]])


@pytest.fixture(scope="module")
def torch_cuda(L):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert L.mi_blur_device_count() >= 1, "libmi_blur.so sees no HIP device"
    torch.cuda.set_device(0)
    return torch


def gpu_conv(pkg, L, torch, host, k, offset_in=0, offset_out=0, y0=None, y1=None):
    """host: N x H x W x C -> mi_blur_enqueue_conv (or _band for one image with y0/y1), guard bytes around the output."""
    n, h, w, c = host.shape
    y0 = 0 if y0 is None else y0
    y1 = h if y1 is None else y1
    size_out = n * (y1 - y0) * w * c
    d_in = torch.zeros(host.size + 64, dtype=torch.uint8, device="cuda")
    d_in[offset_in:offset_in + host.size] = torch.from_numpy(np.ascontiguousarray(host).reshape(-1)).cuda()
    d_out = torch.full((size_out + 128,), 0x5A, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if y0 == 0 and y1 == h:
        rc = L.mi_blur_enqueue_conv(d_in.data_ptr() + offset_in, d_out.data_ptr() + offset_out, w, h, c, n, C.byref(k), s)
    else:
        assert n == 1
        rc = L.mi_blur_enqueue_conv_band(d_in.data_ptr() + offset_in, d_out.data_ptr() + offset_out, w, h, c, y0, y1, C.byref(k), s)
    pkg.check(rc, "mi_blur_enqueue_conv")
    torch.cuda.synchronize()
    o = d_out.cpu().numpy()
    assert (o[:offset_out] == 0x5A).all() and (o[offset_out + size_out:] == 0x5A).all(), "wrote outside the output"
    return o[offset_out:offset_out + size_out].reshape(n, y1 - y0, w, c)


def cpu_conv(pkg, L, img, k):
    a = np.ascontiguousarray(img)
    out = np.empty_like(a)
    n, h, w, c = a.shape
    pkg.check(L.mi_blur_cpu_run_conv(a.ctypes.data, out.ctypes.data, w, h, c, n, C.byref(k), 8))
    return out


def seam_image(rng, h, w, c):
    """Low-amplitude noise with impulses (0 / 255, one channel each) and 0/255 step edges on both sides of every seam
    between tiles (rows and chunk columns) and on the image's borders."""
    cpr = w * c // 16
    nstrips = -(-cpr // TILE_CHUNKS) if cpr else 1
    ncols = -(-cpr // nstrips) if cpr else 1
    rows = sorted({0, h - 1} | {y for s in range(TILE_ROWS, h, TILE_ROWS) for y in (s - 1, s)})
    cols = sorted({0, w - 1} | {min(max(x, 0), w - 1) for s in range(ncols, cpr, ncols) for x in ((s * 16 - 1) // c, -(-s * 16 // c))})
    img = rng.integers(118, 139, size=(2, h, w, c), dtype=np.uint8)
    k = 0
    for y in rows:
        for x in cols:
            img[0, y, x, k % c] = 255 if k % 2 else 0
            k += 1
    for s in rows[1:-1:2]:                                       # a step along every row seam ...
        img[1, s:, : w // 2] = 255
        img[1, :s, w // 2:] = 0
    for s in cols[1:-1:2]:                                       # ... and along every column seam
        img[1, : h // 3, s:] = 255 - img[1, : h // 3, s:]
    return img


# rows of whole 16-byte chunks with 1-4 channels (the tiled kernel at every radius pair) and everything else
ALIGNED = {1: (2, 70, 1040), 2: (1, 65, 536), 3: (2, 66, 688), 4: (1, 40, 272)}        # c -> (n, h, w): several tiles both ways
RAGGED = [(1, 17, 33, 3), (2, 30, 250, 3), (1, 9, 5, 1), (1, 31, 29, 2), (1, 50, 7, 5), (1, 24, 64, 5), (1, 1, 1, 3), (1, 12, 16, 6), (1, 3, 15, 1)]


def test_tiled_kernel_every_radius_pair_channel_count_and_mode(pkg, L, torch_cuda):
    rng = np.random.default_rng(2024)
    assert {p[0] for p in PAIRS} == set(range(8)) and {p[1] for p in PAIRS} == set(range(8))
    for c, (n, h, w) in ALIGNED.items():
        imgs = [rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8), seam_image(rng, h, w, c)]
        for (rx, ry) in PAIRS:
            for mode in cr.MODES:
                spec = cr.random_kernel(rng, rx, ry, zeros=0.2, mode=mode)
                k = cr.make_kernel(pkg, **spec)
                for q, img in enumerate(imgs):
                    got = gpu_conv(pkg, L, torch_cuda, img, k)
                    assert L.mi_blur_last_kernel().decode() == TILED, (c, rx, ry)
                    assert np.array_equal(got, ref_conv(img, **spec)), (c, rx, ry, mode, q)
                    assert np.array_equal(got, cpu_conv(pkg, L, img, k)), (c, rx, ry, mode, q)


def test_tile_edges(pkg, L, torch_cuda):
    """Heights and widths around the tile's row and chunk-column counts (one less, equal, one more, two tiles plus one)."""
    rng = np.random.default_rng(8)
    for c in (1, 3):
        for a, h in enumerate((TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, 2 * TILE_ROWS + 1)):
            for b, chunks in enumerate((TILE_CHUNKS - 1, TILE_CHUNKS, TILE_CHUNKS + 1, 2 * TILE_CHUNKS + 1)):
                w = chunks * 16                                  # cpr = chunks * c: rows of whole chunks whatever the channel count
                img = seam_image(rng, h, w, c)
                for (rx, ry, mode) in (((1, 1, "mag"), (4, 7, "sat"), (7, 2, "abs")), ((2, 3, "sat"), (5, 5, "mag")),
                                       ((3, 6, "abs"), (6, 1, "sat")), ((7, 7, "mag"), (0, 4, "abs")))[(a + b) % 4]:
                    spec = cr.random_kernel(rng, rx, ry, zeros=0.2, mode=mode)
                    got = gpu_conv(pkg, L, torch_cuda, img, cr.make_kernel(pkg, **spec))
                    assert L.mi_blur_last_kernel().decode() == TILED
                    assert np.array_equal(got, ref_conv(img, **spec)), (h, w, c, rx, ry, mode)


def test_generic_kernel(pkg, L, torch_cuda):
    rng = np.random.default_rng(4)
    for (n, h, w, c) in RAGGED:
        img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
        for q, (rx, ry) in enumerate(PAIRS):
            spec = cr.random_kernel(rng, rx, ry, zeros=0.3 * (q % 2), mode=cr.MODES[q % 3])
            got = gpu_conv(pkg, L, torch_cuda, img, cr.make_kernel(pkg, **spec))
            assert L.mi_blur_last_kernel().decode() == GENERIC, ((n, h, w, c), rx, ry)
            assert np.array_equal(got, ref_conv(img, **spec)), ((n, h, w, c), rx, ry)


def test_unaligned_pointers_take_the_generic_kernel(pkg, L, torch_cuda):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(2, 40, 64, 3), dtype=np.uint8)
    for (rx, ry, mode) in ((1, 1, "mag"), (3, 2, "sat"), (7, 7, "abs")):
        spec = cr.random_kernel(rng, rx, ry, mode=mode)
        k = cr.make_kernel(pkg, **spec)
        want = ref_conv(img, **spec)
        assert np.array_equal(gpu_conv(pkg, L, torch_cuda, img, k), want)
        assert L.mi_blur_last_kernel().decode() == TILED
        for oi, oo in ((1, 0), (0, 7), (3, 5)):
            assert np.array_equal(gpu_conv(pkg, L, torch_cuda, img, k, oi, oo), want), (rx, ry, oi, oo)
            assert L.mi_blur_last_kernel().decode() == GENERIC


def test_bands_inside_the_image(pkg, L, torch_cuda):
    rng = np.random.default_rng(12)
    for (h, w, c) in ((64, 80, 3), (37, 17, 3), (90, 64, 4), (40, 48, 1)):
        img = rng.integers(0, 256, size=(1, h, w, c), dtype=np.uint8)
        for (rx, ry, mode) in ((1, 1, "mag"), (2, 2, "sat"), (3, 5, "abs"), (7, 7, "sat")):
            spec = cr.random_kernel(rng, rx, ry, zeros=0.2, mode=mode)
            k = cr.make_kernel(pkg, **spec)
            whole = ref_conv(img, **spec)
            for y0, y1 in ((ry, h - ry), (0, h // 2), (h // 3, h), (5, 6)):
                got = gpu_conv(pkg, L, torch_cuda, img, k, y0=y0, y1=y1)
                assert np.array_equal(got, whole[:, y0:y1]), (h, w, c, rx, ry, y0, y1)
            for split in (ry, h // 2, h - ry):                   # a band split with halo ry, joined, is the whole image
                top_rows = min(h, split + ry)
                top = gpu_conv(pkg, L, torch_cuda, np.ascontiguousarray(img[:, :top_rows]), k, y0=0, y1=split)
                b0 = max(split - ry, 0)
                bot = gpu_conv(pkg, L, torch_cuda, np.ascontiguousarray(img[:, b0:]), k, y0=split - b0, y1=h - b0)
                assert np.array_equal(np.concatenate([top, bot], axis=1), whole), (h, w, c, rx, ry, split)


def test_batch_over_2gib(pkg, L, torch_cuda):
    """A batch of more than 2^31 bytes: 64-bit image offsets, the last image checked."""
    torch = torch_cuda
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, size=(1, 1024, 1024, 3), dtype=np.uint8)
    n = 720                                                   # 2.26 GB in, as much out
    d_in = torch.from_numpy(img[0]).cuda().unsqueeze(0).repeat(n, 1, 1, 1)
    d_in[n - 1, 100:200, 300:400] = 255                       # the last image differs from the others
    last = d_in[n - 1].cpu().numpy()[None]
    d_out = torch.zeros_like(d_in)
    k = cr.make_kernel(pkg, **SOBEL)
    pkg.check(L.mi_blur_enqueue_conv(d_in.data_ptr(), d_out.data_ptr(), 1024, 1024, 3, n, C.byref(k), None))
    torch.cuda.synchronize()
    assert L.mi_blur_last_kernel().decode() == TILED
    want0 = torch.from_numpy(ref_conv(img, **SOBEL)[0]).cuda()
    for i in (0, n // 2, n - 2):
        assert bool((d_out[i] == want0).all()), i
    assert np.array_equal(d_out[n - 1].cpu().numpy(), ref_conv(last, **SOBEL)[0])
    del d_in, d_out
    torch.cuda.empty_cache()


def test_refusals_and_empty_batch(pkg, L, torch_cuda):
    d = torch_cuda.zeros(4096, dtype=torch_cuda.uint8, device="cuda")
    p, q = d.data_ptr(), d.data_ptr() + 2048
    good = pkg.Conv.preset("sobel_mag")
    for field, v in (("rx", 8), ("ry", -1), ("mode", 3), ("shift", 17), ("bias", 2 ** 24 + 1)):
        bad = pkg.Conv.preset("sobel_mag")
        setattr(bad, field, v)
        assert L.mi_blur_enqueue_conv(p, q, 16, 8, 3, 1, C.byref(bad), None) == pkg.ERR_INVALID, field
        assert L.mi_blur_enqueue_conv_band(p, q, 16, 8, 3, 0, 8, C.byref(bad), None) == pkg.ERR_INVALID, field
    bad = pkg.Conv.preset("sobel_mag")
    bad.k2[4] = 32767
    bad.k2[5] = 32767                                            # sum |K2| = 65542
    assert L.mi_blur_enqueue_conv(p, q, 16, 8, 3, 1, C.byref(bad), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_conv(p, q, 16, 8, 3, 1, None, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_conv(p, p, 16, 8, 3, 1, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_conv(None, q, 16, 8, 3, 1, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_conv(p, q, 0, 8, 3, 1, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_conv(p, q, 16, 8, 3, -1, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_conv_band(p, q, 16, 8, 3, 6, 2, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_conv_band(p, q, 16, 8, 3, 0, 9, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_conv(p, q, 16, 8, 3, 0, C.byref(good), None) == pkg.OK
    torch_cuda.cuda.synchronize()


def test_saturation_and_floor_on_both_kernels(pkg, L, torch_cuda):
    for c, (h, w), kernel in ((1, (40, 64), TILED), (3, (33, 48), TILED), (1, (20, 31), GENERIC), (3, (17, 19), GENERIC)):
        for q, (img, spec) in enumerate(cr.saturation_cases(h, w, c)):
            got = gpu_conv(pkg, L, torch_cuda, img, cr.make_kernel(pkg, **spec))
            assert L.mi_blur_last_kernel().decode() == kernel
            assert np.array_equal(got, ref_conv(img, **spec)), (c, kernel, q, spec["mode"], spec["shift"], spec["bias"])


def test_zero_padded_and_all_zero_kernels(pkg, L, torch_cuda):
    rng = np.random.default_rng(10)
    img = rng.integers(0, 256, size=(1, 40, 64, 3), dtype=np.uint8)
    spec = cr.random_kernel(rng, 2, 1, mode="mag")
    a = gpu_conv(pkg, L, torch_cuda, img, cr.make_kernel(pkg, **spec))
    assert np.array_equal(a, ref_conv(img, **spec))
    for (rx, ry) in ((3, 1), (2, 4), (5, 6), (7, 7)):            # other column classes, more rows
        big = dict(spec)
        for t in ("K", "K2"):
            big[t] = np.zeros((2 * ry + 1, 2 * rx + 1), np.int64)
            big[t][ry - 1:ry + 2, rx - 2:rx + 3] = spec[t]
        assert np.array_equal(gpu_conv(pkg, L, torch_cuda, img, cr.make_kernel(pkg, **big)), a), (rx, ry)
    Z = np.zeros((7, 9), np.int64)
    for shift, bias in ((0, 77), (0, 300), (0, -5), (4, 2047)):
        got = gpu_conv(pkg, L, torch_cuda, img, cr.make_kernel(pkg, Z, shift, bias))
        assert (got == min(max(bias >> shift, 0), 255)).all()


def test_gpu_and_cpu_agree_on_the_synthetic_stream(pkg, L, torch_cuda):
    n, h, w, c = 200, 256, 256, 3
    host = np.empty((n, h, w, c), np.uint8)
    L.mi_blur_fill_synthetic(host.ctypes.data, w, h, c, 0, n, 8)
    rng = np.random.default_rng(17)
    random_7x5 = cr.random_kernel(rng, 3, 2, mode="sat")         # 7 columns x 5 rows
    assert random_7x5["K"].shape == (5, 7)
    for k in (pkg.Conv.preset("sobel_mag"), pkg.Conv.preset("sharpen"), cr.make_kernel(pkg, **random_7x5)):
        want = np.empty_like(host)
        pkg.check(L.mi_blur_cpu_run_conv(host.ctypes.data, want.ctypes.data, w, h, c, n, C.byref(k), 16))
        assert np.array_equal(gpu_conv(pkg, L, torch_cuda, host, k), want)
        assert L.mi_blur_last_kernel().decode() == TILED


def test_context_with_a_conv(pkg, L, torch_cuda):
    """Every submit form of a GPU context takes the filter: pageable, pinned (one launch: not the batch server), strided
    bands, one band, planar."""
    rng = np.random.default_rng(21)
    n, h, w, c = 6, 240, 320, 3                                # 1.38 MB of output per submit: the server size class
    img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    isz = img[0].size
    for spec in (SOBEL, cr.random_kernel(rng, 3, 2, zeros=0.3, mode="sat"), cr.random_kernel(rng, 7, 7, mode="abs")):
        r = np.asarray(spec["K"]).shape[0] // 2
        want = ref_conv(img, **spec)
        with pkg.Context(0, w, h, c, 1, max_batch=n, n_slots=3) as ctx:
            ctx.set_conv(cr.make_kernel(pkg, **spec))
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
            ctx.submit_bands(img.ctypes.data + (60 - r) * pitch, bo.ctypes.data + 60 * pitch, n, isz, 120 + 2 * r, r, r)
            ctx.sync()
            assert np.array_equal(bo[:, 60:180], want[:, 60:180]) and not bo[:, :60].any() and not bo[:, 180:].any()
            so = np.zeros((100, w, c), np.uint8)
            ctx.submit_band(img[1].ctypes.data + (50 - r) * pitch, so.ctypes.data, 100 + 2 * r, r, r)
            ctx.sync()
            assert np.array_equal(so, want[1, 50:150])
            planar = np.ascontiguousarray(img.transpose(0, 3, 1, 2))
            po = np.zeros_like(img)
            ctx.submit_planar(planar.ctypes.data, po.ctypes.data, n)
            ctx.sync()
            assert np.array_equal(po, want)
            assert L.mi_blur_ctx_set_conv(ctx.h, C.byref(cr.make_kernel(pkg, **spec))) == pkg.ERR_STATE
            ctx.resident_alloc(2)
            assert L.mi_blur_resident_run(ctx.h, 2, 1, 0) == pkg.ERR_UNSUPPORTED
            assert L.mi_blur_resident_run_fused(ctx.h, 2, 1, 0) == pkg.ERR_UNSUPPORTED


def test_python_functions(pkg, torch_cuda):
    rng = np.random.default_rng(30)
    imgs = rng.integers(0, 256, size=(4, 90, 128, 3), dtype=np.uint8)
    cpu = pkg.DEVICE_CPU
    assert np.array_equal(pkg.sobel(imgs), ref_conv(imgs, **SOBEL))
    for axis in ("x", "y", "mag"):
        assert np.array_equal(pkg.sobel(imgs, axis), pkg.sobel(imgs, axis, device=cpu)), axis
        assert np.array_equal(pkg.scharr(imgs, axis, batch=3), pkg.scharr(imgs, axis, device=cpu)), axis
    for conn in (4, 8):
        assert np.array_equal(pkg.laplacian(imgs, conn), pkg.laplacian(imgs, conn, device=cpu))
    assert np.array_equal(pkg.sharpen(imgs), ref_conv(imgs, **SHARPEN))
    spec = cr.random_kernel(rng, 5, 3, mode="mag")
    got = pkg.filter2d(imgs, spec["K"], spec["shift"], spec["bias"], "mag", spec["K2"])
    assert np.array_equal(got, ref_conv(imgs, **spec))
    assert np.array_equal(got, pkg.filter2d(imgs, spec["K"], spec["shift"], spec["bias"], "mag", spec["K2"], device=cpu))
    g = imgs[0, :, :, 0]
    got = pkg.sobel(g)
    assert got.shape == g.shape and np.array_equal(got, ref_conv(g[None, :, :, None], **SOBEL)[0, :, :, 0])


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


def test_hosts_conv_on_the_gpu(pkg, torch_cuda, tmp_path):
    pkg.build_native()
    het, spl = os.path.join(pkg.APPS, "heterogeneous_blur"), os.path.join(pkg.APPS, "split_image_blur")
    rng = np.random.default_rng(40)
    img = rng.integers(0, 256, size=(240, 320, 3), dtype=np.uint8)
    write_ppm(tmp_path / "in.ppm", img)
    emboss = dict(K=[[-2, -1, 0], [-1, 1, 1], [0, 1, 2]], bias=128)
    for name, spec in (("sobel", SOBEL), ("emboss", emboss)):
        want = ref_conv(img[None], **spec)[0]
        for mode in ("gpu", "both"):
            out = f"{mode}_{name}.ppm"
            r = subprocess.run([het, mode, "0.7", "35", "--image", "in.ppm", "--images", "100", "--conv", name, "--save", out],
                               cwd=tmp_path, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout + r.stderr
            assert f"Blur kernel: 3x3 convolution ({name})\n" in r.stdout
            assert np.array_equal(read_ppm(tmp_path / out), want), (mode, name)
    r = subprocess.run([spl, "0.6", "16", "--image", "in.ppm", "--images", "48", "--conv", "sharpen", "--save", "s.ppm"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Halo size: 1 row(s)" in r.stdout and "Blur kernel: 3x3 convolution (sharpen)\n" in r.stdout
    assert np.array_equal(read_ppm(tmp_path / "s.ppm"), ref_conv(img[None], **SHARPEN)[0])
