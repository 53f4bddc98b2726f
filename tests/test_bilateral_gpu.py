"""Bilateral filter on a real MI355X (-m gpu): mi_blur_enqueue_bilateral / _band, a context given the filter by
mi_blur_ctx_set_bilateral, bilateral_filter() and the hosts' --bilateral, byte for byte against the numpy restatement of
the definition in include/mi_blur.h (bilateral_ref.py) and against the CPU device.  0x5A guard bytes surround every output."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bilateral_ref as br
from bilateral_ref import ref_bilateral

pytestmark = pytest.mark.gpu

TILED, GENERIC = "blur_bilateral_tiled_kernel", "blur_bilateral_generic_kernel"
TILE_ROWS, TILE_CHUNKS = 32, 32                                   # blur_bilateral_tiled_kernel's tile: output rows x 16-byte chunk columns
RADII = tuple(range(1, 9))


@pytest.fixture(scope="module")
def torch_cuda(L):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert L.mi_blur_device_count() >= 1, "libmi_blur.so sees no HIP device"
    torch.cuda.set_device(0)
    return torch


def gpu_bilateral(pkg, L, torch, host, k, offset_in=0, offset_out=0, y0=None, y1=None):
    """host: N x H x W x C -> mi_blur_enqueue_bilateral (or _band for one image with y0/y1), guard bytes around the output."""
    n, h, w, c = host.shape
    y0 = 0 if y0 is None else y0
    y1 = h if y1 is None else y1
    size_out = n * (y1 - y0) * w * c
    d_in = torch.zeros(host.size + 64, dtype=torch.uint8, device="cuda")
    d_in[offset_in:offset_in + host.size] = torch.from_numpy(np.ascontiguousarray(host).reshape(-1)).cuda()
    d_out = torch.full((size_out + 128,), 0x5A, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if y0 == 0 and y1 == h:
        rc = L.mi_blur_enqueue_bilateral(d_in.data_ptr() + offset_in, d_out.data_ptr() + offset_out, w, h, c, n, C.byref(k), s)
    else:
        assert n == 1
        rc = L.mi_blur_enqueue_bilateral_band(d_in.data_ptr() + offset_in, d_out.data_ptr() + offset_out, w, h, c, y0, y1, C.byref(k), s)
    pkg.check(rc, "mi_blur_enqueue_bilateral")
    torch.cuda.synchronize()
    o = d_out.cpu().numpy()
    assert (o[:offset_out] == 0x5A).all() and (o[offset_out + size_out:] == 0x5A).all(), "wrote outside the output"
    return o[offset_out:offset_out + size_out].reshape(n, y1 - y0, w, c)


def cpu_bilateral(pkg, L, img, k):
    a = np.ascontiguousarray(img)
    out = np.empty_like(a)
    n, h, w, c = a.shape
    pkg.check(L.mi_blur_cpu_run_bilateral(a.ctypes.data, out.ctypes.data, w, h, c, n, C.byref(k), 8))
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


# rows of whole 16-byte chunks with 1-4 channels (the tiled kernel at every radius) and everything else
ALIGNED = {1: (2, 70, 1040), 2: (1, 65, 536), 3: (2, 66, 688), 4: (1, 40, 272)}        # c -> (n, h, w): several tiles both ways
RAGGED = [(1, 17, 33, 3), (2, 30, 250, 3), (1, 9, 5, 1), (1, 31, 29, 2), (1, 50, 7, 5), (1, 24, 64, 5), (1, 1, 1, 3), (1, 12, 16, 6), (1, 3, 15, 1)]


def test_tiled_kernel_every_radius_and_channel_count(pkg, L, torch_cuda):
    rng = np.random.default_rng(2024)
    for c, (n, h, w) in ALIGNED.items():
        imgs = [rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8), seam_image(rng, h, w, c)]
        for r in RADII:
            for t, tables in enumerate((br.gauss_tables(0, 25.0, r), br.random_tables(rng, r, zeros=0.3))):
                k = br.make_kernel(pkg, *tables)
                for q, img in enumerate(imgs):
                    got = gpu_bilateral(pkg, L, torch_cuda, img, k)
                    assert L.mi_blur_last_kernel().decode() == TILED, (c, r)
                    assert np.array_equal(got, ref_bilateral(img, *tables)), (c, r, t, q)
                    assert np.array_equal(got, cpu_bilateral(pkg, L, img, k)), (c, r, t, q)


def test_tile_edges(pkg, L, torch_cuda):
    """Heights and widths around the tile's row and chunk-column counts (one less, equal, one more, two tiles plus one)."""
    rng = np.random.default_rng(8)
    for c in (1, 3):
        for a, h in enumerate((TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, 2 * TILE_ROWS + 1)):
            for b, chunks in enumerate((TILE_CHUNKS - 1, TILE_CHUNKS, TILE_CHUNKS + 1, 2 * TILE_CHUNKS + 1)):
                w = chunks * 16                                  # cpr = chunks * c: rows of whole chunks whatever the channel count
                img = seam_image(rng, h, w, c)
                for r in ((1, 4, 8), (2, 5), (3, 6), (7,))[(a + b) % 4]:
                    tables = br.random_tables(rng, r, zeros=0.2)
                    got = gpu_bilateral(pkg, L, torch_cuda, img, br.make_kernel(pkg, *tables))
                    assert L.mi_blur_last_kernel().decode() == TILED
                    assert np.array_equal(got, ref_bilateral(img, *tables)), (h, w, c, r)


def test_input_kinds(pkg, L, torch_cuda):
    rng = np.random.default_rng(3)
    for (n, h, w, c) in ((1, 50, 96, 3), (2, 37, 64, 1)):
        for q, img in enumerate(br.input_kinds(rng, n, h, w, c)):
            for r in (1, 2, 4, 8):
                for tables in (br.gauss_tables(0, 12.0, r), br.random_tables(rng, r)):
                    got = gpu_bilateral(pkg, L, torch_cuda, img, br.make_kernel(pkg, *tables))
                    assert L.mi_blur_last_kernel().decode() == TILED
                    assert np.array_equal(got, ref_bilateral(img, *tables)), ((n, h, w, c), q, r)


def test_generic_kernel(pkg, L, torch_cuda):
    rng = np.random.default_rng(4)
    for (n, h, w, c) in RAGGED:
        img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
        for r in RADII:
            tables = br.random_tables(rng, r, zeros=0.3) if r % 2 else br.gauss_tables(0, 30.0, r)
            got = gpu_bilateral(pkg, L, torch_cuda, img, br.make_kernel(pkg, *tables))
            assert L.mi_blur_last_kernel().decode() == GENERIC, ((n, h, w, c), r)
            assert np.array_equal(got, ref_bilateral(img, *tables)), ((n, h, w, c), r)


def test_unaligned_pointers_take_the_generic_kernel(pkg, L, torch_cuda):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(2, 40, 64, 3), dtype=np.uint8)
    for r in (1, 3, 8):
        tables = br.random_tables(rng, r)
        k = br.make_kernel(pkg, *tables)
        want = ref_bilateral(img, *tables)
        assert np.array_equal(gpu_bilateral(pkg, L, torch_cuda, img, k), want)
        assert L.mi_blur_last_kernel().decode() == TILED
        for oi, oo in ((1, 0), (0, 7), (3, 5)):
            assert np.array_equal(gpu_bilateral(pkg, L, torch_cuda, img, k, oi, oo), want), (r, oi, oo)
            assert L.mi_blur_last_kernel().decode() == GENERIC


def test_bands_inside_the_image(pkg, L, torch_cuda):
    rng = np.random.default_rng(12)
    for (h, w, c) in ((64, 80, 3), (37, 17, 3), (90, 64, 4), (40, 48, 1)):
        img = rng.integers(0, 256, size=(1, h, w, c), dtype=np.uint8)
        for r in (1, 2, 5, 8):
            tables = br.random_tables(rng, r, zeros=0.2)
            k = br.make_kernel(pkg, *tables)
            whole = ref_bilateral(img, *tables)
            for y0, y1 in ((r, h - r), (0, h // 2), (h // 3, h), (5, 6)):
                got = gpu_bilateral(pkg, L, torch_cuda, img, k, y0=y0, y1=y1)
                assert np.array_equal(got, whole[:, y0:y1]), (h, w, c, r, y0, y1)
            for split in (r, h // 2, h - r):                     # a band split with halo r, joined, is the whole image
                top_rows = min(h, split + r)
                top = gpu_bilateral(pkg, L, torch_cuda, np.ascontiguousarray(img[:, :top_rows]), k, y0=0, y1=split)
                b0 = max(split - r, 0)
                bot = gpu_bilateral(pkg, L, torch_cuda, np.ascontiguousarray(img[:, b0:]), k, y0=split - b0, y1=h - b0)
                assert np.array_equal(np.concatenate([top, bot], axis=1), whole), (h, w, c, r, split)


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
    tables = br.gauss_tables(0, 25.0, 1)
    k = br.make_kernel(pkg, *tables)
    pkg.check(L.mi_blur_enqueue_bilateral(d_in.data_ptr(), d_out.data_ptr(), 1024, 1024, 3, n, C.byref(k), None))
    torch.cuda.synchronize()
    assert L.mi_blur_last_kernel().decode() == TILED
    want0 = torch.from_numpy(ref_bilateral(img, *tables)[0]).cuda()
    for i in (0, n // 2, n - 2):
        assert bool((d_out[i] == want0).all()), i
    assert np.array_equal(d_out[n - 1].cpu().numpy(), ref_bilateral(last, *tables)[0])
    del d_in, d_out
    torch.cuda.empty_cache()


def test_refusals_and_empty_batch(pkg, L, torch_cuda):
    d = torch_cuda.zeros(4096, dtype=torch_cuda.uint8, device="cuda")
    p, q = d.data_ptr(), d.data_ptr() + 2048
    good = pkg.Bilateral.gauss(0.0, 25.0, 2)
    bad = pkg.Bilateral.gauss(0.0, 25.0, 2)
    bad.radius = 9
    assert L.mi_blur_enqueue_bilateral(p, q, 16, 8, 3, 1, C.byref(bad), None) == pkg.ERR_INVALID
    bad.radius, bad.range[0] = 2, 0
    assert L.mi_blur_enqueue_bilateral(p, q, 16, 8, 3, 1, C.byref(bad), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_bilateral(p, q, 16, 8, 3, 1, None, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_bilateral(p, p, 16, 8, 3, 1, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_bilateral(None, q, 16, 8, 3, 1, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_bilateral(p, q, 0, 8, 3, 1, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_bilateral(p, q, 16, 8, 3, -1, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_bilateral_band(p, q, 16, 8, 3, 6, 2, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_bilateral_band(p, q, 16, 8, 3, 0, 9, C.byref(good), None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_bilateral(p, q, 16, 8, 3, 0, C.byref(good), None) == pkg.OK
    torch_cuda.cuda.synchronize()


def test_division_boundaries(pkg, L, torch_cuda):
    """Two-valued windows whose counts step through every split, S all 1 and R all 255: quotients on and beside .5; then
    random tables on the same images and on random bytes, where num / den is arbitrary."""
    rng = np.random.default_rng(6)
    ones = np.full(256, 255, np.int64)
    for (h, w, c) in ((64, 128, 1), (40, 80, 2)):
        img = br.division_images(h, w, c)
        for r in RADII:
            S = np.ones((2 * r + 1, 2 * r + 1), np.int64)
            for tables in ((S, ones), (S * 3, ones // 5), br.random_tables(rng, r)):
                got = gpu_bilateral(pkg, L, torch_cuda, img, br.make_kernel(pkg, *tables))
                assert L.mi_blur_last_kernel().decode() == TILED
                assert np.array_equal(got, ref_bilateral(img, *tables)), (h, w, c, r)
    # the largest sums the validation admits
    S = np.full((17, 17), 226, np.int64)
    S.reshape(-1)[:65535 - 226 * 289] += 1
    for img in (np.full((1, 40, 64, 1), 255, np.uint8), rng.integers(200, 256, size=(1, 40, 64, 1), dtype=np.uint8),
                rng.integers(0, 256, size=(1, 40, 64, 1), dtype=np.uint8)):
        got = gpu_bilateral(pkg, L, torch_cuda, img, br.make_kernel(pkg, S, ones))
        assert np.array_equal(got, ref_bilateral(img, S, ones))
        got = gpu_bilateral(pkg, L, torch_cuda, img[:, :, :63], br.make_kernel(pkg, S, ones))       # the generic kernel's division
        assert L.mi_blur_last_kernel().decode() == GENERIC
        assert np.array_equal(got, ref_bilateral(img[:, :, :63], S, ones))


def test_gpu_and_cpu_agree_on_the_synthetic_stream(pkg, L, torch_cuda):
    n, h, w, c = 200, 256, 256, 3
    host = np.empty((n, h, w, c), np.uint8)
    L.mi_blur_fill_synthetic(host.ctypes.data, w, h, c, 0, n, 8)
    for r in (1, 2, 4):
        k = pkg.Bilateral.gauss(0.0, 25.0, r)
        want = np.empty_like(host)
        pkg.check(L.mi_blur_cpu_run_bilateral(host.ctypes.data, want.ctypes.data, w, h, c, n, C.byref(k), 16))
        assert np.array_equal(gpu_bilateral(pkg, L, torch_cuda, host, k), want), r


def test_context_with_a_bilateral(pkg, L, torch_cuda):
    """Every submit form of a GPU context takes the filter: pageable, pinned (one launch: not the batch server), strided
    bands, one band, planar."""
    rng = np.random.default_rng(21)
    n, h, w, c = 6, 240, 320, 3                                # 1.38 MB of output per submit: the server size class
    img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    isz = img[0].size
    for r, tables in ((1, br.gauss_tables(0, 25.0, 1)), (3, br.random_tables(rng, 3, zeros=0.3)), (8, br.gauss_tables(0, 40.0, 8))):
        want = ref_bilateral(img, *tables)
        with pkg.Context(0, w, h, c, 1, max_batch=n, n_slots=3) as ctx:
            ctx.set_bilateral(br.make_kernel(pkg, *tables))
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
            assert L.mi_blur_ctx_set_bilateral(ctx.h, C.byref(br.make_kernel(pkg, *tables))) == pkg.ERR_STATE
            ctx.resident_alloc(2)
            assert L.mi_blur_resident_run(ctx.h, 2, 1, 0) == pkg.ERR_UNSUPPORTED
            assert L.mi_blur_resident_run_fused(ctx.h, 2, 1, 0) == pkg.ERR_UNSUPPORTED


def test_bilateral_filter_python(pkg, torch_cuda):
    rng = np.random.default_rng(30)
    imgs = rng.integers(0, 256, size=(4, 90, 128, 3), dtype=np.uint8)
    for k in (3, 5, 9, 17):
        assert np.array_equal(pkg.bilateral_filter(imgs, k), ref_bilateral(imgs, *br.gauss_tables(k / 4.0, 25.0, k // 2))), k
    assert np.array_equal(pkg.bilateral_filter(imgs, 7, sigma_color=50.0, sigma_space=3.0, batch=3), ref_bilateral(imgs, *br.gauss_tables(3.0, 50.0, 3)))
    g = imgs[0, :, :, 0]
    assert np.array_equal(pkg.bilateral_filter(g, 5), ref_bilateral(g[None, :, :, None], *br.gauss_tables(1.25, 25.0, 2))[0, :, :, 0])
    assert np.array_equal(pkg.bilateral_filter(imgs, 5), pkg.bilateral_filter(imgs, 5, device=pkg.DEVICE_CPU))


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


def test_hosts_bilateral_on_the_gpu(pkg, torch_cuda, tmp_path):
    pkg.build_native()
    het, spl = os.path.join(pkg.APPS, "heterogeneous_blur"), os.path.join(pkg.APPS, "split_image_blur")
    rng = np.random.default_rng(40)
    img = rng.integers(0, 256, size=(240, 320, 3), dtype=np.uint8)
    write_ppm(tmp_path / "in.ppm", img)
    for k, extra, sc, ss in ((5, [], 25.0, 1.25), (17, ["--sigma-color", "40", "--sigma-space", "5"], 40.0, 5.0)):
        want = ref_bilateral(img[None], *br.gauss_tables(ss, sc, k // 2))[0]
        for mode in ("gpu", "both"):
            out = f"{mode}{k}.ppm"
            r = subprocess.run([het, mode, "0.7", "35", "--image", "in.ppm", "--images", "100", "--bilateral", str(k)] + extra +
                               ["--save", out], cwd=tmp_path, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout + r.stderr
            assert f"Blur kernel: {k}x{k} bilateral (sigma_color {sc:g}, sigma_space {ss:g})\n" in r.stdout
            assert np.array_equal(read_ppm(tmp_path / out), want), (mode, k)
    r = subprocess.run([spl, "0.6", "16", "--image", "in.ppm", "--images", "48", "--bilateral", "7", "--save", "s.ppm"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Halo size: 3 row(s)" in r.stdout and "Blur kernel: 7x7 bilateral (sigma_color 25, sigma_space 1.75)\n" in r.stdout
    assert np.array_equal(read_ppm(tmp_path / "s.ppm"), ref_bilateral(img[None], *br.gauss_tables(1.75, 25.0, 3))[0])
